"""CAPTURE_VIDEO on the host side: the camera, the palette and the frame ring of the step-observer protocol (utils/observers.py).

The frames are drawn on the device by ``vine_render_scheduled`` (include/vine_render.h), a launch behind every step that
decides from the device's step counter whether the step just finished belongs to a capture window.  The window harvest is
``observers.WindowRing``'s; the writer thread encodes the APNG (utils/apng.py)."""
import os

import numpy as np
import torch

from .. import abi, native
from .apng import write_apng
from .observers import WindowRing, capture_schedule  # noqa: F401  (capture_schedule: importable from here as before)


def render_config(lib, env_cfg, centre_y, centre_z):
    """``VineRenderConfig`` from the task's ``env`` block: the reference's camera unless a CAPTURE_VIDEO_* key says
    otherwise."""
    c = abi.VineRenderConfig()
    native.check(lib.vine_render_config_default(c), lib)
    c.capture_every = int(env_cfg.get("CAPTURE_VIDEO_EVERY", c.capture_every))
    c.num_frames = int(env_cfg.get("CAPTURE_VIDEO_FRAMES", c.num_frames))
    c.num_views = int(env_cfg.get("CAPTURE_VIDEO_VIEWS", c.num_views))
    c.width = int(env_cfg.get("CAPTURE_VIDEO_WIDTH", c.width))
    c.height = int(env_cfg.get("CAPTURE_VIDEO_HEIGHT", c.height))
    c.grid_cols = int(np.ceil(np.sqrt(c.num_views)))
    c.centre_y, c.centre_z = float(centre_y), float(centre_z)
    return c


def palette(lib):
    import ctypes as C
    buf = (C.c_uint8 * (3 * abi.VR_NUM_MATERIALS))()
    n = C.c_int(0)
    native.check(lib.vine_render_palette(buf, C.byref(n)), lib)
    return np.frombuffer(bytes(buf), dtype=np.uint8).reshape(n.value, 3).copy()


class VideoCapture(WindowRing):
    """The frame ring of one env handle: a ``WindowRing`` of ``rcfg.num_frames`` frames every ``rcfg.capture_every`` steps."""

    SKIPPED, WRITER = "Video", "video"

    def __init__(self, lib, handle, rcfg, view_envs, progress_buf, device, directory, time_str, frame_delay,
                 logger=None):
        self.lib, self.handle, self.rcfg = lib, handle, rcfg
        self.directory, self.time_str, self.frame_delay = directory, time_str, float(frame_delay)
        nbytes = int(lib.vine_render_ring_bytes(rcfg))
        if nbytes < 0:
            native.check(nbytes, lib)
        self.frame_shape = rcfg.frame_shape
        self.view_envs = torch.as_tensor(list(view_envs), dtype=torch.int32, device=device)
        self.progress_buf = progress_buf
        self.ring = torch.zeros((rcfg.num_frames,) + self.frame_shape, dtype=torch.uint8, device=device)
        assert self.ring.numel() == nbytes
        self.host = torch.empty(self.ring.shape, dtype=torch.uint8, pin_memory=True)
        self.palette = palette(lib)
        self.on_frames = None        # test hook: called in the writer thread with (frames, last) before encoding
        super().__init__(device, logger)

    def live_tensors(self):
        return []                    # no caller rolls the frame ring back: a replay redraws every slot before it is harvested

    def enqueue(self, stream, actions=None):
        """The scheduled draw, behind the step just enqueued on ``stream`` (captured with it inside a hipGraph).
        (The picture has no use for ``actions``.)"""
        native.check(self.lib.vine_render_scheduled(self.handle, self.rcfg, self.view_envs.data_ptr(),
                                                    self.progress_buf.data_ptr(), self.ring.data_ptr(), stream), self.lib)

    def _window(self):
        return self.rcfg.capture_every, self.rcfg.num_frames

    def _copies(self):
        return [(self.ring, self.host)]

    def _write(self, start, last, extra):
        frames = self.host.numpy()
        if self.on_frames is not None:
            self.on_frames(frames.copy(), last)
        os.makedirs(self.directory, exist_ok=True)
        path = os.path.join(self.directory, f"{self.time_str}_video_{last}.png")
        self.logger.info("-" * 100)
        self.logger.info(f"Saving video to {path}...")
        write_apng(path, frames, self.palette, self.frame_delay)
        self.written.append(path)
        self.logger.info("DONE")
        self.logger.info("-" * 100)
