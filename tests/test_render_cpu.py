"""CAPTURE_VIDEO without a GPU: the APNG writer, the float64 reference renderer on hand-made states, the capture
schedule against a literal restatement of the reference's loop, and the C ABI of include/vine_render.h."""
import ctypes as C
import os
import re
import struct
import zlib

import numpy as np
import pytest

from tests import render_reference as rr
from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import apng
from vine_robot_isaacgymenvs_amd.utils.video import capture_schedule

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- APNG
def _random_video(seed=0, n=7, h=33, w=50, colours=12):
    rng = np.random.default_rng(seed)
    return rng.integers(0, colours, (n, h, w), dtype=np.uint8), rng.integers(0, 256, (colours, 3), dtype=np.uint8)


def test_apng_round_trip(tmp_path):
    frames, palette = _random_video()
    path = apng.write_apng(str(tmp_path / "v.png"), frames, palette, (333, 10000))
    got, pal, delays = apng.read_apng(path)
    assert got.dtype == np.uint8 and np.array_equal(got, frames)
    assert np.array_equal(pal, palette)
    assert delays == [(333, 10000)] * len(frames)
    assert apng.delay_fraction(0.03332) == (333, 10000)
    assert not os.path.exists(path + ".part")


def test_apng_chunks_crc_and_sequence(tmp_path):
    """Walks the file by hand: every CRC matches, fcTL / fdAT carry one running sequence number, frame 0 is an IDAT."""
    frames, palette = _random_video(1, n=4)
    blob = open(apng.write_apng(str(tmp_path / "v.png"), frames, palette, 0.05), "rb").read()
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    pos, kinds, seqs = 8, [], []
    while pos < len(blob):
        (length,) = struct.unpack(">I", blob[pos:pos + 4])
        kind, payload = blob[pos + 4:pos + 8], blob[pos + 8:pos + 8 + length]
        assert struct.unpack(">I", blob[pos + 8 + length:pos + 12 + length])[0] == zlib.crc32(kind + payload) & 0xFFFFFFFF
        kinds.append(kind)
        if kind in (b"fcTL", b"fdAT"):
            seqs.append(struct.unpack(">I", payload[:4])[0])
        pos += 12 + length
    assert kinds == [b"IHDR", b"PLTE", b"acTL", b"fcTL", b"IDAT"] + [b"fcTL", b"fdAT"] * 3 + [b"IEND"]
    assert seqs == list(range(7))


def test_apng_reader_rejects_a_damaged_file(tmp_path):
    frames, palette = _random_video(2, n=2)
    path = apng.write_apng(str(tmp_path / "v.png"), frames, palette, 0.05)
    blob = bytearray(open(path, "rb").read())
    blob[len(blob) // 2] ^= 0x40
    open(path, "wb").write(bytes(blob))
    with pytest.raises((ValueError, zlib.error)):
        apng.read_apng(path)


def test_apng_opens_in_pil(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    frames, palette = _random_video(3)
    path = apng.write_apng(str(tmp_path / "v.png"), frames, palette, 0.05)
    im = Image.open(path)
    assert im.n_frames == len(frames)
    for i in (0, len(frames) - 1):
        im.seek(i)
        assert np.array_equal(np.asarray(im.convert("RGB")), palette[frames[i]])


# ------------------------------------------------------------------------------------------- the reference renderer
PARAMS = dict(flags=0, link_length=0.0885, joint1_z=0.965, phi0=np.pi, rail_soft_limit=0.35, success_dist=0.04,
              max_episode_length=500)
VIEW = dict(width=400, height=225, centre_y=0.0, centre_z=1.0, metres_per_pixel=0.005)


def _state(q=(0.0,) * 6, target=(0.3, 0.6)):
    st = np.zeros((abi.VF_COUNT, 1))
    st[abi.VF_Q0:abi.VF_Q0 + 6, 0] = q
    st[abi.VF_TARGET_Y, 0], st[abi.VF_TARGET_Z, 0] = target
    st[abi.VF_SHELF_Y, 0], st[abi.VF_SHELF_Z, 0] = 0.25, 0.65
    st[abi.VF_PIPE_Y, 0], st[abi.VF_PIPE_Z, 0], st[abi.VF_OBJ_ANGLE, 0] = -0.35, 0.55, -1.2
    return st


def test_reference_tip_and_target_pixels():
    st = _state(q=(0.1, 0.3, -0.2, 0.25, 0.1, -0.15))
    img, _ = rr.render(st, 0, PARAMS, VIEW)
    ty, tz = rr.tip_position(st, 0, PARAMS)
    assert img[rr.pixel_of(VIEW, ty, tz)] == abi.VR_TIP
    assert img[rr.pixel_of(VIEW, 0.3, 0.6)] == abi.VR_TARGET
    assert img[0, 0] == abi.VR_BACKGROUND


def test_reference_straight_vine_is_a_vertical_bar():
    """All joint angles 0 (phi0 = pi): the links hang straight down from joint1_z as one bar.  Its lateral extent is the
    link rectangle's [-0.0381, 0.0719] mirrored by the half turn, i.e. y in [-0.0719, 0.0381] around the cart."""
    img, _ = rr.render(_state(), 0, PARAMS, VIEW)
    Y, Z = rr.pixel_centres(VIEW)
    link = (img == abi.VR_LINK_A) | (img == abi.VR_LINK_B)
    bottom = 0.965 - 5 * 0.0885
    rows = np.where((Z[:, 0] < 0.965 - 0.02) & (Z[:, 0] > bottom + 0.02))[0]       # clear of the cart and of the tip disc
    assert len(rows) > 50
    expect = (Y[0] > -0.0719) & (Y[0] < 0.0381)
    assert expect.sum() == 22                                                       # 0.11 m of 5 mm pixels
    for r in rows:
        assert np.array_equal(link[r], expect), r
    assert not link[Z[:, 0] < bottom - 0.001].any()
    assert not link[Z[:, 0] > 0.965 + 0.00575 + 0.001].any()
    # the two shades alternate down the bar
    col = rr.pixel_of(VIEW, 0.0, 1.0)[1]
    shades = [img[rr.pixel_of(VIEW, 0.0, 0.965 - (k + 0.5) * 0.0885)[0], col] for k in range(5)]
    assert shades == [abi.VR_LINK_A, abi.VR_LINK_B, abi.VR_LINK_A, abi.VR_LINK_B, abi.VR_LINK_A]


def test_reference_obstacles_follow_their_flags():
    st = _state()
    free, _ = rr.render(st, 0, PARAMS, VIEW)
    assert not np.isin(free, (abi.VR_SHELF, abi.VR_STRIP, abi.VR_PIPE)).any()
    shelf, _ = rr.render(st, 0, dict(PARAMS, flags=abi.FLAG_CREATE_SHELF), VIEW)
    assert (shelf == abi.VR_SHELF).sum() > 100 and not (shelf == abi.VR_PIPE).any()
    # the strip is 2 mm wide: at 5 mm a pixel it shows only where a pixel centre falls inside it; at 1 mm a pixel always
    fine, _ = rr.render(st, 0, dict(PARAMS, flags=abi.FLAG_CREATE_SHELF), dict(VIEW, metres_per_pixel=0.001, centre_y=0.4, centre_z=0.6505))
    assert (fine == abi.VR_STRIP).sum() == 2 * 10
    assert shelf[rr.pixel_of(VIEW, 0.25, 0.65 + 0.2)] == abi.VR_SHELF                # the upper board's centre
    pipe, _ = rr.render(st, 0, dict(PARAMS, flags=abi.FLAG_CREATE_PIPE), VIEW)
    assert (pipe == abi.VR_PIPE).sum() > 50 and not np.isin(pipe, (abi.VR_SHELF, abi.VR_STRIP)).any()


def test_reference_progress_bar_length():
    st = _state()
    none, _ = rr.render(st, 0, PARAMS, VIEW)
    assert not (none == abi.VR_PROGRESS).any()
    Y, _ = rr.pixel_centres(VIEW)
    for progress in (125, 250, 500):
        img, _ = rr.render(st, 0, PARAMS, VIEW, progress=progress)
        bar = img == abi.VR_PROGRESS
        rows = np.where(bar.any(1))[0]
        assert len(rows) == 3                         # 2.5 px around z = 1.2, a row of pixel centres at this height
        ys = Y[0][bar[rows[0]]]
        assert abs(ys.min() - (-0.4 + 0.0025)) < 1e-9
        assert np.array_equal(bar[rows[0]], bar[rows[2]])
        assert abs(ys.max() - (-0.4 + 0.8 * progress / 500 - 0.0025)) < 1e-9


def test_reference_distance_field():
    """The distance is measured to the nearest boundary of any shape."""
    img, dist = rr.render(_state(), 0, PARAMS, VIEW)
    r, c = rr.pixel_of(VIEW, 0.0, 0.975)
    assert img[r, c + 9] == abi.VR_CART                  # y = 0.0475: right of the links (they end at y = 0.0381) ...
    assert abs(dist[r, c + 9] - 0.0025) < 1e-9           # ... and 2.5 mm from the cart's right edge y = 0.05
    assert dist.min() >= 0.0


# ---------------------------------------------------------------------------------------------------------- schedule
def _reference_loop(first_step, n_steps, capture_every, num_frames):
    """V5:1170-1207 restated literally: ``video_frames`` holds the step indices instead of images."""
    num_steps, video_frames, drawn, saved = first_step, [], [], []
    for _ in range(n_steps):
        should_start = num_steps % capture_every == 0
        in_progress = len(video_frames) > 0
        if should_start or in_progress:
            drawn.append((num_steps, len(video_frames)))
            video_frames.append(num_steps)
            if len(video_frames) == num_frames:
                saved.append((video_frames[0], num_steps))
                video_frames = []
        num_steps += 1
    return drawn, saved


@pytest.mark.parametrize("first,every,frames,chunk", [(0, 1000, 100, 16), (0, 40, 10, 16), (7, 40, 10, 16), (25, 40, 10, 1),
                                                      (40, 40, 10, 16), (0, 40, 24, 16), (3, 48, 16, 16), (0, 37, 37, 5), (990, 1000, 100, 16)])
def test_schedule_matches_the_reference_loop(first, every, frames, chunk):
    total = 3200
    drawn, saved = _reference_loop(first, total, every, frames)
    got_draws, got_done, done = [], [], first
    while done < first + total:
        draws, completed, opens = capture_schedule(done, chunk, every, frames, valid_from=first)
        assert opens == any(slot == 0 for _, slot in draws)
        got_draws += draws
        got_done += completed
        done += chunk
    # a count that starts inside a window: the device draws that window's remaining slots, the reference does not (it is
    # not capturing) -- and neither saves it
    start = first if first % every == 0 else (first // every + 1) * every
    assert [d for d in got_draws if d[0] >= start] == drawn
    assert all(s % every < frames for s, _ in got_draws)
    assert got_done == saved
    if chunk == 16 and every == 40:
        assert any((s // chunk) != (last // chunk) for s, last in saved)           # windows that straddle rollouts
        if frames == 24:
            assert any(last % chunk == chunk - 1 for _, last in saved)             # one ends on a rollout's last step


# --------------------------------------------------------------------------------------------------------------- ABI
def _header():
    return open(os.path.join(REPO, "include", "vine_render.h")).read()


def _header_functions():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(vine_[a-z_0-9]+)\s*\(", text)))


@pytest.fixture(scope="module")
def hip_lib():
    native.build()
    return native.load()


def test_render_header_and_ctypes_mirror_agree(hip_lib):
    names = _header_functions()
    assert names == sorted(abi.RENDER_PROTOTYPES)
    for name in names:
        assert hasattr(hip_lib, name), name
    assert hip_lib.vine_render_config_size() == C.sizeof(abi.VineRenderConfig)
    text = _header()
    fields = re.findall(r"^\s+(?:int32_t|float)\s+([a-z_, ]+);", re.search(r"typedef struct VineRenderConfig \{(.*?)\}", text, re.S).group(1),
                        re.M)
    names = [n.strip() for group in fields for n in group.split(",")]
    assert names == [n for n, _ in abi.VineRenderConfig._fields_]
    assert int(re.search(r"#define VINE_RENDER_ABI_VERSION (\d+)", text).group(1)) == abi.RENDER_ABI_VERSION
    assert float(re.search(r"#define VINE_RENDER_LINE_PX ([0-9.]+)f", text).group(1)) == abi.RENDER_LINE_PX == rr.LINE_PX
    assert float(re.search(r"#define VINE_RENDER_TIP_RADIUS ([0-9.]+)f", text).group(1)) == abi.RENDER_TIP_RADIUS == rr.TIP_RADIUS
    enum = re.findall(r"\b(VR_[A-Z_]+) = (\d+)", text)
    assert [(k, int(v)) for k, v in enum] == [(k, getattr(abi, k)) for k, _ in enum] and len(enum) == abi.VR_NUM_MATERIALS + 1


def test_render_defaults_sizes_and_palette(hip_lib):
    c = abi.VineRenderConfig()
    assert hip_lib.vine_render_config_default(c) == abi.OK
    assert (c.abi_version, c.width, c.height, c.num_views, c.grid_cols, c.num_frames, c.capture_every) == (1, 400, 225, 1, 1, 100, 1000)
    assert (c.centre_y, c.centre_z) == (0.0, 1.0) and c.metres_per_pixel == np.float32(2.0 / 400)
    assert hip_lib.vine_render_frame_bytes(c) == 400 * 225 and hip_lib.vine_render_ring_bytes(c) == 100 * 400 * 225
    c.num_views, c.grid_cols = 7, 3
    assert c.frame_shape == (3 * 225, 3 * 400) and hip_lib.vine_render_frame_bytes(c) == 9 * 400 * 225
    c.grid_cols = 8
    assert hip_lib.vine_render_frame_bytes(c) == abi.ERR_INVALID_ARG and b"grid_cols" in hip_lib.vine_last_error()
    buf = (C.c_uint8 * (3 * abi.VR_NUM_MATERIALS))()
    n = C.c_int(0)
    assert hip_lib.vine_render_palette(buf, C.byref(n)) == abi.OK and n.value == abi.VR_NUM_MATERIALS
    pal = np.frombuffer(bytes(buf), np.uint8).reshape(-1, 3)
    assert len({tuple(p) for p in pal}) == abi.VR_NUM_MATERIALS             # every material its own colour
    assert tuple(pal[abi.VR_LIMIT]) == (230, 26, 26) and tuple(pal[abi.VR_PROGRESS]) == (26, 230, 26)   # V5:1149, 1164
    assert len(abi.RENDER_MATERIAL_NAMES) == abi.VR_NUM_MATERIALS
