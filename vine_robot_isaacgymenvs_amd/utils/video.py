"""CAPTURE_VIDEO on the host side: the schedule arithmetic and the harvest of the device frame ring.

The frames are drawn on the device by ``vine_render_scheduled`` (include/vine_render.h), a launch behind every step that
decides from the device's step counter whether the step just finished belongs to a capture window.  The host never asks
the device where it is: it counts the steps it has enqueued (``VideoCapture.advance``), and ``capture_schedule`` tells it
which windows those steps completed.  A completed window is copied to pinned host memory on a side stream and handed to a
writer thread that encodes the APNG (utils/apng.py); the training loop never waits for the encoder."""
import logging
import os
import queue
import threading

import numpy as np
import torch

from .. import abi, native
from .apng import write_apng


def capture_schedule(steps_done, n_steps, capture_every, num_frames, valid_from=0):
    """What ``n_steps`` more steps do to the capture, when ``steps_done`` steps have been completed before them.

    The step with index s (the s-th step since the count was 0, counted from 0) is drawn into slot ``s % capture_every``
    iff that is ``< num_frames``: the reference opens a window when ``num_steps % capture_video_every == 0``, keeps
    appending while one is in progress, saves when it holds ``num_video_frames`` frames, and increments ``num_steps``
    after all that (V5:1170-1207).

    Returns ``(draws, completed, opens)``:
      draws      [(s, slot)] of the steps among the new ones that are drawn
      completed  [(start, last)] of the windows whose LAST frame is among the new steps and whose first frame was drawn
                 at or after step ``valid_from`` (a step count set into the middle of a window leaves that window's
                 early slots undrawn: the reference would not be capturing either); ``last`` is the reference's
                 ``num_steps`` at the moment it saves, the number in the file name
      opens      True when one of the new steps is the first frame of a window (slot 0 is overwritten)
    """
    lo, hi = int(steps_done), int(steps_done) + int(n_steps)       # the new steps are lo .. hi - 1
    every, frames = int(capture_every), int(num_frames)
    draws, completed, opens = [], [], False
    w = lo // every                                                # the window whose range may reach into [lo, hi)
    while w * every < hi:
        start = w * every
        for s in range(max(start, lo), min(start + frames, hi)):
            draws.append((s, s - start))
        if lo <= start < hi:
            opens = True
        last = start + frames - 1
        if lo <= last < hi and start >= valid_from:
            completed.append((start, last))
        w += 1
    return draws, completed, opens


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


class VideoCapture:
    """The frame ring of one env handle, the host's count of its steps, and the harvest."""

    def __init__(self, lib, handle, rcfg, view_envs, progress_buf, device, directory, time_str, frame_delay,
                 logger=None):
        self.lib, self.handle, self.rcfg, self.device = lib, handle, rcfg, device
        self.logger = logger or logging.getLogger(__name__)
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
        self.steps_done = 0          # the device's step count, as the host knows it from what it has enqueued
        self.valid_from = 0
        self.paused = 0
        self.side = torch.cuda.Stream(device=device)
        self.copy_done = None        # event behind the last ring -> host copy, until the ring may be overwritten again
        self.host_free = threading.Event()
        self.host_free.set()
        self.jobs = queue.Queue()
        self.written, self.skipped = [], []
        self.on_frames = None        # test hook: called in the writer thread with (frames, last) before encoding
        self.writer = threading.Thread(target=self._write_loop, name="vine-video-writer", daemon=True)
        self.writer.start()

    # -- device side -------------------------------------------------------------------------------------------------
    def enqueue(self, stream, actions=None):
        """The scheduled draw, behind the step just enqueued on ``stream`` (captured with it inside a hipGraph).
        (``actions``, the step's action buffer, is what the task hands every step observer; the picture has no use for it.)"""
        native.check(self.lib.vine_render_scheduled(self.handle, self.rcfg, self.view_envs.data_ptr(),
                                                    self.progress_buf.data_ptr(), self.ring.data_ptr(), stream), self.lib)

    # -- host side ---------------------------------------------------------------------------------------------------
    def set_steps(self, steps):
        """The step count was set from outside (tests; the restore behind a graph's warm-up pass): windows already open
        at that count are not complete.  (Setting the count the host already has is no discontinuity.)"""
        if int(steps) == self.steps_done:
            return
        self.steps_done = int(steps)
        self.valid_from = int(steps)

    def before(self, n_steps):
        """Call before enqueueing ``n_steps`` steps: if they open a window, the copy of the previous one must be
        complete before slot 0 is drawn again (it finished long ago in practice)."""
        if self.paused or self.copy_done is None:
            return
        _, _, opens = capture_schedule(self.steps_done, n_steps, self.rcfg.capture_every, self.rcfg.num_frames)
        if opens:
            torch.cuda.current_stream(self.device).wait_event(self.copy_done)
            self.copy_done = None

    def advance(self, n_steps):
        """Call after enqueueing ``n_steps`` steps (each with its scheduled draw behind it)."""
        if self.paused:
            return
        _, completed, _ = capture_schedule(self.steps_done, n_steps, self.rcfg.capture_every, self.rcfg.num_frames,
                                           self.valid_from)
        self.steps_done += int(n_steps)
        for start, last in completed:
            if self.steps_done > start + self.rcfg.capture_every:
                self._skip(last, "the next window began within the same batch of steps")
            else:
                self._harvest(last)

    def _skip(self, last, why):
        self.skipped.append(last)
        self.logger.info(f"Video of the window ending at step {last} not saved: {why}")

    def _harvest(self, last):
        if not self.host_free.is_set():
            self._skip(last, "the writer still holds the host buffer")
            return
        self.host_free.clear()
        main = torch.cuda.current_stream(self.device)
        drawn = torch.cuda.Event()
        drawn.record(main)
        self.side.wait_event(drawn)
        with torch.cuda.stream(self.side):
            self.host.copy_(self.ring, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.side)
        self.copy_done = done
        self.jobs.put((done, last))

    def _write_loop(self):
        while True:
            job = self.jobs.get()
            if job is None:
                return
            done, last = job
            try:
                done.synchronize()
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
            except Exception:                     # the training loop does not die of a full disk
                self.logger.exception("video writer failed")
            finally:
                self.host_free.set()

    def drain(self):
        """Wait until every harvested window is on disk."""
        self.host_free.wait()          # at most one window is in flight: the buffer is taken before its job is queued

    def close(self):
        if self.writer is not None:
            self.jobs.put(None)
            self.writer.join()
            self.writer = None
