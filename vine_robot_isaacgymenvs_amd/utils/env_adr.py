"""ENV_PARAMS_ADR on the host side: the step observer whose two launches behind every step widen or narrow the ranges an
env's plant is redrawn from (``vine_env_adr_scheduled``, include/vine_env_adr.h), the host's complete copy of the history of
those moves, and the scalars a trainer logs.

``EnvAdr`` takes ``env_redraw.EnvRedraw``'s place, last in launch order.  The ranges of the names under ADR begin at START;
the ``[lo, hi]`` of ``ENV_PARAMS`` are the limits.  All state is integers on the device; ``env_params.adr_replay`` is the
host statement of both launches, and ``env_params.adr_episode_columns`` rebuilds the plant of any episode from the history."""
import numpy as np
import torch

from .. import abi, native
from . import env_params
from .env_redraw import EnvRedraw


class EnvAdr(EnvRedraw):
    """A step observer (the protocol: utils/observers.py), last in launch order like the redraw it replaces."""

    def __init__(self, lib, handle, vcfg, spec, adr, reset, params, inertia, device, logger=None):
        """``spec``: the ENV_PARAMS mapping (the limits); ``adr``: ``env_params.adr_config``'s result; the rest as for
        ``EnvRedraw``.  ``params`` / ``inertia`` hold episode 0: the tables of ``env_params.adr_start_spec``.  A reward
        matrix must be bound to ``handle`` before the first step."""
        super().__init__(lib, handle, vcfg, spec, reset, params, inertia, device)
        import logging
        self.logger = logger or logging.getLogger(__name__)
        self.adr = adr
        self.aspec = env_params.adr_spec(lib, vcfg, self.spec, adr, self.values.data_ptr() if self.values is not None else None)
        n = params.shape[1]
        self._ints = torch.zeros(abi.VR_NAMES * 6, dtype=torch.int32, device=device)      # widen, then counts: one copy reads both
        self.widen = self._ints[:abi.VR_NAMES * 2].view(abi.VR_NAMES, 2)
        self.counts = self._ints[abi.VR_NAMES * 2:].view(abi.VR_NAMES, 2, 2)
        self.widen0 = np.zeros((abi.VR_NAMES, 2), dtype=np.int64)      # what was in force before the first step (a restored checkpoint's)
        self.reached = torch.zeros(n, dtype=torch.int32, device=device)
        self.probe = torch.full((n,), -1, dtype=torch.int32, device=device)
        self.capacity = int(adr["HISTORY_CAPACITY"])
        self.history = torch.zeros((self.capacity, abi.ENV_ADR_HISTORY_WORDS), dtype=torch.int32, device=device)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=device)
        self.history_rows = np.zeros((0, abi.ENV_ADR_HISTORY_WORDS), dtype=np.int64)      # every row harvested so far
        self.history_harvested = 0       # the cursor at the last harvest
        self.history_dropped = 0
        self._scalars = torch.zeros(abi.VR_NAMES * 6, dtype=torch.int32).pin_memory()      # widen, then counts

    # -- the observer protocol ---------------------------------------------------------------------------------------------
    def enqueue(self, stream, actions=None):
        native.check(self.lib.vine_env_adr_scheduled(
            self.handle, self.aspec, self.reset.data_ptr(), self.params.data_ptr(),
            self.inertia.data_ptr() if self.inertia is not None else None, self.episode_index.data_ptr(), self.widen.data_ptr(),
            self.counts.data_ptr(), self.reached.data_ptr(), self.probe.data_ptr(), self.history.data_ptr(),
            self.cursor.data_ptr(), stream), self.lib)

    def live_tensors(self):
        """A rolled-back pass has moved all of it.  The history ring is not among them: what the pass appends lies past the
        restored cursor, where later rows overwrite it."""
        return super().live_tensors() + [self._ints, self.reached, self.probe, self.cursor]

    def reset_envs(self, env_ids):
        """The envs were reset from outside the step: they keep their plant and their episode ordinal, and that episode is
        no longer counted at a boundary.  The log does not know: the row that episode later writes still reports, in its
        ``probe`` column, the boundary its plant was DRAWN at (``param_*`` stays right, the plant is kept)."""
        self.reached[env_ids] = 0
        self.probe[env_ids] = -1

    # -- the history -------------------------------------------------------------------------------------------------------
    def harvest_history(self):
        """Copy the history rows appended since the last harvest (synchronises).  Returns the complete history [H, 4]."""
        if torch.cuda.is_current_stream_capturing():
            return self.history_rows
        cursor = int(self.cursor.item())
        lost = max(0, cursor - self.history_harvested - self.capacity)
        if lost:
            self.history_dropped += lost
            self.logger.warning(f"ENV_PARAMS_ADR: {lost} history rows were overwritten before they were harvested "
                                f"({self.history_dropped} in all): raise ENV_PARAMS_ADR.HISTORY_CAPACITY")
        first = max(self.history_harvested, cursor - self.capacity)
        self.history_harvested = cursor
        if cursor > first:
            a, b = first % self.capacity, (cursor - 1) % self.capacity + 1
            rows = self.history[a:b] if a < b else torch.cat([self.history[a:], self.history[:b]])
            self.history_rows = np.concatenate([self.history_rows, rows.cpu().numpy().astype(np.int64)])
        return self.history_rows

    # -- which plant -------------------------------------------------------------------------------------------------------
    def columns(self, envs, episodes):
        raise RuntimeError("ENV_PARAMS_ADR: an episode's plant also depends on the step that drew it: episode_columns()")

    def episode_columns(self, envs, episodes, drawn_at):
        """``env_params.adr_episode_columns`` of local env indices ``envs``: ``(params, inertia or None, probe)``, float64 with
        NaN where ``drawn_at`` is -1, from the history harvested so far; no device involved."""
        gids = np.asarray(envs, dtype=np.int64) + self.env_id_offset
        return env_params.adr_episode_columns(self.spec, self.adr, self.seed, gids, episodes, drawn_at, self.history_rows,
                                              vcfg=self.vcfg, lib=self.lib, widen0=self.widen0)

    # -- what a trainer logs -----------------------------------------------------------------------------------------------
    def scalars(self):
        """``{"adr/<NAME>_lo": .., "adr/<NAME>_hi": .., "adr/probing_reach_rate": ..}`` at this point of the current stream:
        one non-blocking copy of ``widen`` and ``counts`` into pinned memory and a wait for it, where the caller
        synchronises anyway.  The rate is that of the probing episodes now in the queues (absent while they are empty)."""
        done = torch.cuda.Event()
        self._scalars.copy_(self._ints, non_blocking=True)
        done.record(torch.cuda.current_stream(self.device))
        done.synchronize()
        host = self._scalars.numpy()
        widen = host[:abi.VR_NAMES * 2].reshape(abi.VR_NAMES, 2)
        counts = host[abi.VR_NAMES * 2:].reshape(abi.VR_NAMES, 2, 2)
        out = {}
        for name, (lo, hi) in env_params.adr_ranges(self.spec, self.adr, widen).items():
            out[f"adr/{name}_lo"], out[f"adr/{name}_hi"] = lo, hi
        if counts[..., 0].sum() > 0:
            out["adr/probing_reach_rate"] = float(counts[..., 1].sum()) / float(counts[..., 0].sum())
        return out

    def state_dict(self):
        """What a checkpoint keeps: ``widen`` (synchronises)."""
        return {"widen": self.widen.cpu().numpy().astype(np.int64), "names": list(self.adr["NAMES"])}

    def load_state_dict(self, state):
        widen = np.asarray(state["widen"], dtype=np.int64).reshape(abi.VR_NAMES, 2)
        limit = env_params.adr_max_widen(self.spec, self.adr)
        if list(state.get("names", self.adr["NAMES"])) != list(self.adr["NAMES"]) or np.any(widen < 0) or np.any(widen > limit):
            raise ValueError("ENV_PARAMS_ADR: the checkpoint's widen does not fit this configuration's NAMES, START, STEP and limits")
        if self.history_harvested or int(self.cursor.item()):
            raise RuntimeError("ENV_PARAMS_ADR: a checkpoint's widen is restored before the first step, not into a run under way")
        self.widen.copy_(torch.as_tensor(widen, dtype=torch.int32))
        self.widen0 = widen.copy()           # the episode log's join starts from it: this run's history has no row for it
