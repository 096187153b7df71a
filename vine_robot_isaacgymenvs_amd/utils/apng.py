"""Animated PNG with an indexed palette, from ``zlib`` and ``struct`` alone.

The reference saves its rollout videos with ``imageio.mimsave(<...>.gif)`` (V5:1190-1200); imageio is not on the target
image, GIF's LZW in pure Python takes seconds for a 100-frame window, and the renderer's frames ARE palette indices
(include/vine_render.h), so the file format here is APNG: every frame is one zlib stream of its rows, compressed at C
speed, with no colour quantisation.  Browsers, wandb and PIL open it; a viewer that only knows PNG shows frame 0.

Layout (PNG 1.2 + the APNG extension): signature, IHDR (8-bit, colour type 3), PLTE, acTL (frame count, loop forever),
then per frame an fcTL (sequence number, size, delay as a fraction of a second) and its data -- IDAT for frame 0, fdAT
(sequence number + the same zlib stream) for the others -- and IEND.  fcTL and fdAT share ONE running sequence number.
``read_apng`` parses such a file back and checks every chunk's CRC and the sequence numbers (tests; quick looks)."""
import os
import struct
import zlib

import numpy as np

_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload) & 0xFFFFFFFF)


def delay_fraction(seconds):
    """Seconds -> (numerator, denominator) of an fcTL delay: ten-thousandths of a second, clamped to what 16 bits hold."""
    return max(1, min(65535, int(round(float(seconds) * 10000.0)))), 10000


def write_apng(path, frames, palette, delay, level=6):
    """frames: uint8 [F, H, W] of palette indices; palette: uint8 [P, 3] RGB with P <= 256 and every index < P;
    delay: seconds per frame, or an exact (numerator, denominator) pair.  Returns ``path``."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    palette = np.ascontiguousarray(palette, dtype=np.uint8)
    if frames.ndim != 3 or frames.shape[0] < 1:
        raise ValueError("frames must be [F, H, W] with F >= 1")
    if palette.ndim != 2 or palette.shape[1] != 3 or not 1 <= palette.shape[0] <= 256:
        raise ValueError("palette must be [P, 3] with 1 <= P <= 256")
    if int(frames.max()) >= palette.shape[0]:
        raise ValueError("a frame holds an index beyond the palette")
    num, den = delay if isinstance(delay, tuple) else delay_fraction(delay)
    n, h, w = frames.shape
    rows = np.zeros((h, w + 1), dtype=np.uint8)          # filter type 0 (none) in front of every row
    out = [_SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 3, 0, 0, 0)), _chunk(b"PLTE", palette.tobytes()),
           _chunk(b"acTL", struct.pack(">II", n, 0))]
    seq = 0
    for i in range(n):
        out.append(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, w, h, 0, 0, num, den, 0, 0)))
        seq += 1
        rows[:, 1:] = frames[i]
        data = zlib.compress(rows.tobytes(), level)
        if i == 0:
            out.append(_chunk(b"IDAT", data))
        else:
            out.append(_chunk(b"fdAT", struct.pack(">I", seq) + data))
            seq += 1
    out.append(_chunk(b"IEND", b""))
    tmp = path + ".part"
    with open(tmp, "wb") as f:                            # a reader never sees half a file under the final name
        f.write(b"".join(out))
    os.replace(tmp, path)
    return path


def read_apng(path):
    """-> (frames uint8 [F, H, W], palette uint8 [P, 3], delays [(numerator, denominator)] * F).  Raises ValueError on a
    bad signature, a chunk whose CRC does not match, a sequence number out of order or a frame count that differs from
    acTL's.  Reads what ``write_apng`` writes: full-size frames, filter type 0."""
    with open(path, "rb") as f:
        blob = f.read()
    if blob[:8] != _SIGNATURE:
        raise ValueError("not a PNG file")
    pos, w, h, palette, declared, seq = 8, None, None, None, None, 0
    streams, delays = [], []
    while pos < len(blob):
        (length,) = struct.unpack(">I", blob[pos:pos + 4])
        kind, payload = blob[pos + 4:pos + 8], blob[pos + 8:pos + 8 + length]
        (crc,) = struct.unpack(">I", blob[pos + 8 + length:pos + 12 + length])
        if crc != (zlib.crc32(kind + payload) & 0xFFFFFFFF):
            raise ValueError("CRC mismatch in chunk %r at byte %d" % (kind, pos))
        pos += 12 + length
        if kind == b"IHDR":
            w, h, depth, ctype, _, _, interlace = struct.unpack(">IIBBBBB", payload)
            if (depth, ctype, interlace) != (8, 3, 0):
                raise ValueError("only 8-bit indexed, non-interlaced images")
        elif kind == b"PLTE":
            palette = np.frombuffer(payload, dtype=np.uint8).reshape(-1, 3).copy()
        elif kind == b"acTL":
            declared, _ = struct.unpack(">II", payload)
        elif kind == b"fcTL":
            s, fw, fh, x0, y0, num, den, _, _ = struct.unpack(">IIIIIHHBB", payload)
            if s != seq or (fw, fh, x0, y0) != (w, h, 0, 0):
                raise ValueError("fcTL out of sequence or not full-size")
            seq += 1
            delays.append((num, den))
            streams.append([])
        elif kind == b"IDAT":
            streams[-1].append(payload)
        elif kind == b"fdAT":
            (s,) = struct.unpack(">I", payload[:4])
            if s != seq:
                raise ValueError("fdAT out of sequence")
            seq += 1
            streams[-1].append(payload[4:])
        elif kind == b"IEND":
            break
    if declared is None or declared != len(streams):
        raise ValueError("acTL declares %r frames, the file holds %d" % (declared, len(streams)))
    frames = np.empty((len(streams), h, w), dtype=np.uint8)
    for i, parts in enumerate(streams):
        rows = np.frombuffer(zlib.decompress(b"".join(parts)), dtype=np.uint8).reshape(h, w + 1)
        if rows[:, 0].any():
            raise ValueError("row filter other than 0")
        frames[i] = rows[:, 1:]
    return frames, palette, delays
