"""Step observers: what rides behind every env step, and the harvest the two windowed ones share.

A step observer is a launch behind every step launch of one env handle (captured with it inside a hipGraph) that decides
from the device's step counter what, if anything, that step means to it, plus the host's own account of the steps it has
enqueued.  The task class (tasks/vine5link_moving_base.py) keeps its observers in one list and calls all of them alike:

  before(n)                 ``n`` steps are about to be enqueued (or a graph holding them replayed)
  enqueue(stream, actions)  the observer's launch behind the step just enqueued on ``stream``; ``actions``: device address
                            of the action buffer that step consumed.  An observer whose class attribute ``wants_obs`` is
                            true is called as ``enqueue(stream, actions, obs=address)`` with the device address of the
                            observation buffer that step wrote; every other observer is called exactly as before, with the
                            two positional arguments, and needs no ``obs`` parameter
  advance(n)                ``n`` steps, each with its launch behind it, have been enqueued (or replayed)
  set_steps(steps)          the device's step count was set from outside
  live_tensors()            what a caller that rolls steps back (the warm-up pass in front of a graph capture) must save
                            and restore
  drain()                   wait until everything harvested is on disk
  close()
  paused                    while non-zero, ``before`` and ``advance`` do nothing: the steps are rolled back or not executed
  copy_done                 event behind a harvest copy still reading the observer's device buffers, else ``None``

The observers: ``video.VideoCapture`` (CAPTURE_VIDEO), ``trajectory.TrajectoryRecorder`` (RECORD_TRAJECTORIES) -- both a
``WindowRing`` --, ``episodes.EpisodeLog`` (EPISODE_LOG), the SYSID node of utils/sysid.py, and, last in launch order,
``env_redraw.EnvRedraw`` (ENV_PARAMS_PER_EPISODE): the one observer that WRITES what the step reads -- the bound per-env
tables and the delay rings of the envs the step has just flagged -- so it runs behind the others, which have then read what
this step's plant produced.  Its ``live_tensors`` are the tables and its episode counters.  Under ENV_PARAMS_ADR
``env_adr.EnvAdr`` stands in its place: two launches that also move the ranges the plants are drawn from, whose integers
(steps per boundary, counts, per-env flags, the history cursor) are live tensors too.  ``env_sensor.EnvSensor`` (ENV_SENSOR)
rewrites the observation the step has just written (``wants_obs``); it reads the step's reset flags and nothing the redraw
writes, and stands in front of the redraw, which stays last.  ``env_push.EnvPush`` (ENV_PUSH) adds impulses to the six
generalised velocities of the state block the step has just written.  It stands behind every observer that reads that block
-- the video, the recorder and the episode log account for the step as the plant left it -- and behind the sensor, and in
front of the redraw: it reads the inertia table's column of the episode that has just run, which the redraw replaces.
``env_target.EnvTarget`` (ENV_TARGET) moves the target in the state block for the NEXT step and adds the target's velocity to
the observation the step has just written (``wants_obs``).  It stands behind the video, the recorder and the episode log,
which must see the target the step used, and in front of the sensor, which then delays and perturbs the velocity columns
with the rest of the frame.  ``env_draw_adr.EnvDrawAdr`` (ENV_DRAW_ADR) moves the ranges the target, the sensor and the push
redraw their values from, and replaces the rows those three have just drawn for a flagged env with the draw from the range in
force: it stands behind all three -- each redraws as the last statement of its launch and reads the new row in a later
launch only -- and in front of the redraw, which stays last.  So the order is: video, recorder, episode log, target, sensor,
push, draw ADR, redraw / ADR.

Those last observers keep no host account of the steps: ``StepObserver`` states the protocol's names that mean nothing to
them once, and ``TableObserver`` what the target, the sensor and the push share -- a per-env table of named draws
(utils/named_draw.py) that their launch redraws at a reset.

The host never asks the device where it is: it counts the steps it has enqueued, and ``capture_schedule`` tells it which
windows those steps completed.  A completed window is copied to pinned host memory on a side stream and handed to a writer
thread; the training loop never waits for the encoder or the disk."""
import collections
import logging
import queue
import threading
import time

import numpy as np
import torch

from . import named_draw


KEEP = 256       # entries of a windowed observer's bookkeeping lists


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


class WindowRing:
    """A device ring that a launch behind every step fills during the first ``length`` steps of every ``period``, the host's
    count of the handle's steps, and the harvest of a completed window.

    A subclass gives ``enqueue``, ``live_tensors``, the nouns of the two log lines (``SKIPPED``, ``WRITER``) and
      _window()                  (period, length) in steps
      _copies()                  the (device tensor, pinned host tensor) pairs of a harvest, looked up at every harvest
      _job_extra()               what rides along with a harvested window to ``_write``
      _write(start, last, extra) in the writer thread, the host tensors complete: write the window's files"""

    SKIPPED = WRITER = None

    def __init__(self, device, logger=None):
        self.device = device
        self.logger = logger or logging.getLogger(__name__)
        self.steps_done = 0          # the device's step count, as the host knows it from what it has enqueued
        self.valid_from = 0
        self.paused = 0
        self.side = torch.cuda.Stream(device=device)
        self.copy_done = None        # event behind the last ring -> host copy, until the ring may be overwritten again
        self.host_free = threading.Event()
        self.host_free.set()
        self.jobs = queue.Queue()
        # the most recent files and skipped windows, and the host cost of the most recent windows (the harvest call, the
        # writer thread); bounded: a long training completes thousands of windows
        self.written, self.skipped = collections.deque(maxlen=KEEP), collections.deque(maxlen=KEEP)
        self.harvest_seconds, self.write_seconds = collections.deque(maxlen=KEEP), collections.deque(maxlen=KEEP)
        self.windows_written = self.windows_skipped = 0
        self.writer = threading.Thread(target=self._write_loop, name=f"vine-{self.WRITER}-writer", daemon=True)
        self.writer.start()

    def _job_extra(self):
        return None

    def set_steps(self, steps):
        """The step count was set from outside (tests; the restore behind a graph's warm-up pass): windows already open
        at that count are not complete.  (Setting the count the host already has is no discontinuity.)"""
        if int(steps) == self.steps_done:
            return
        self.steps_done = int(steps)
        self.valid_from = int(steps)

    def before(self, n_steps):
        """Call before enqueueing ``n_steps`` steps: if they open a window, the copy of the previous one must be
        complete before slot 0 is written again (it finished long ago in practice)."""
        if self.paused or self.copy_done is None:
            return
        _, _, opens = capture_schedule(self.steps_done, n_steps, *self._window())
        if opens:
            torch.cuda.current_stream(self.device).wait_event(self.copy_done)
            self.copy_done = None

    def advance(self, n_steps):
        """Call after enqueueing ``n_steps`` steps (each with its scheduled launch behind it)."""
        if self.paused:
            return
        period, length = self._window()
        _, completed, _ = capture_schedule(self.steps_done, n_steps, period, length, self.valid_from)
        self.steps_done += int(n_steps)
        for start, last in completed:
            if self.steps_done > start + period:
                self._skip(last, "the next window began within the same batch of steps")
            else:
                self._harvest(start, last)

    def _skip(self, last, why):
        self.skipped.append(last)
        self.windows_skipped += 1
        self.logger.info(f"{self.SKIPPED} of the window ending at step {last} not saved: {why}")

    def _harvest(self, start, last):
        if not self.host_free.is_set():
            self._skip(last, "the writer still holds the host buffer")
            return
        t0 = time.perf_counter()
        self.host_free.clear()
        main = torch.cuda.current_stream(self.device)
        filled = torch.cuda.Event()
        filled.record(main)
        self.side.wait_event(filled)
        with torch.cuda.stream(self.side):
            for ring, host in self._copies():
                host.copy_(ring, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.side)
        self.copy_done = done
        self.jobs.put((done, start, last, self._job_extra()))
        self.harvest_seconds.append(time.perf_counter() - t0)

    def _write_loop(self):
        while True:
            job = self.jobs.get()
            if job is None:
                return
            done, start, last, extra = job
            try:
                done.synchronize()
                t0 = time.perf_counter()
                self._write(start, last, extra)
                self.write_seconds.append(time.perf_counter() - t0)
                self.windows_written += 1
            except Exception:                     # the training loop does not die of a full disk
                self.logger.exception(f"{self.WRITER} writer failed")
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


class StepObserver:
    """An observer whose launch follows the device's own counters: the host has nothing to count, wait for or write, so the
    protocol's ``before``, ``advance``, ``set_steps``, ``drain`` and ``close`` do nothing.  A subclass gives ``enqueue`` and
    ``live_tensors`` and owns ``episode_index`` (int32 [N] on the device)."""

    def __init__(self):
        self.paused = 0
        self.copy_done = None

    def before(self, n_steps):
        pass

    def advance(self, n_steps):
        pass

    def set_steps(self, steps):
        pass

    def drain(self):
        pass

    def close(self):
        pass

    def episodes_now(self):
        """A host copy of ``episode_index`` at this point of the current stream (synchronises)."""
        return self.episode_index.cpu().numpy().astype(np.int64)


class TableObserver(StepObserver):
    """A step observer with a float32 ``table`` [len(NAMES), N] of named draws (utils/named_draw.py), one row per name of the
    checked ``spec``: episode 0's draw, which the observer's launch replaces per env at a reset when the spec says
    ``PER_EPISODE`` (counting the env's episodes in ``episode_index``).  A subclass states ``NAMES`` (the spec's keys, the
    table's rows), ``DRAW_NAMES`` (what the draw is keyed by, and the log's ``param_`` columns) and ``INTEGER`` (the draw
    names whose range is over the integers), checks the spec against ``values_ptr`` and adds its own buffers."""

    NAMES = DRAW_NAMES = INTEGER = ()

    def __init__(self, lib, handle, vcfg, spec, num_envs, device):
        super().__init__()
        self.lib, self.handle, self.vcfg, self.device = lib, handle, vcfg, device
        self.spec = spec
        self.seed, self.env_id_offset = int(vcfg.seed), int(vcfg.env_id_offset)
        self.num_envs = int(num_envs)
        named = named_draw.named(self.NAMES, self.DRAW_NAMES, spec)
        values = named_draw.pack(named)[1]
        self.values = torch.as_tensor(values, dtype=torch.float64, device=device) if len(values) else None
        gids = np.arange(self.num_envs, dtype=np.int64) + self.env_id_offset
        self.table = torch.as_tensor(named_draw.draw(named, self.seed, gids, 0, self.INTEGER).astype(np.float32),
                                     device=device).contiguous()
        self.episode_index = torch.zeros(self.num_envs, dtype=torch.int32, device=device)

    @property
    def values_ptr(self):
        """The device address of the value lists, ``None`` when the spec has none."""
        return self.values.data_ptr() if self.values is not None else None

    def episode_params(self, envs, episodes):
        """``named_draw.episode_params`` of local env indices ``envs``."""
        return named_draw.episode_params(self.NAMES, self.DRAW_NAMES, self.spec, self.seed,
                                         np.asarray(envs, dtype=np.int64) + self.env_id_offset, episodes, self.INTEGER)


class FirstFrameObserver(TableObserver):
    """A ``TableObserver`` whose launch treats the first frame of an episode specially and so must hear of a reset from
    outside the step: ``fresh`` (uint8 [N]), set here, cleared by the launch."""

    def __init__(self, lib, handle, vcfg, spec, num_envs, device):
        super().__init__(lib, handle, vcfg, spec, num_envs, device)
        self.fresh = torch.ones(self.num_envs, dtype=torch.uint8, device=device)

    def reset_envs(self, env_ids):
        """The envs were reset from outside the step: the next frame of each is its episode's first."""
        self.fresh[env_ids] = 1
