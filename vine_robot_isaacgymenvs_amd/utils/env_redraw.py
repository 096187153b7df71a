"""ENV_PARAMS_PER_EPISODE on the host side: the step observer whose launch behind every step redraws the plant of the envs
that step has flagged for a reset (``vine_env_redraw_scheduled``, include/vine_env_redraw.h), and the host's knowledge of
which plant an episode ran with.

The device keeps ``episode_index`` (int32 [N]): the ordinal of the episode every env is in, 0 until its first reset from
inside the step.  Episode ``k`` of global env ``g`` runs with ``env_params.draw_columns(spec, ..., [g], [k])``; the host never
mirrors the tables, it recomputes a column from ``(g, k)`` when somebody asks (the episode log's ``param_*`` columns), or
reads the device (``columns``)."""
import numpy as np
import torch

from .. import native
from . import env_params
from .observers import StepObserver


class EnvRedraw(StepObserver):
    """A step observer (the protocol: utils/observers.py), last in launch order: the step's other observers have read what
    the step wrote before the next step's plant replaces this one's."""

    def __init__(self, lib, handle, vcfg, spec, reset, params, inertia, device):
        """``reset``: the step's reset buffer; ``params`` / ``inertia``: the device tensors bound to ``handle`` (``inertia``
        ``None`` when the spec names no mass)."""
        super().__init__()
        self.lib, self.handle, self.vcfg, self.device = lib, handle, vcfg, device
        self.spec = env_params.spec_forms(spec)      # as plain numbers and lists: what the episode file stores as JSON
        self.seed, self.env_id_offset = int(vcfg.seed), int(vcfg.env_id_offset)
        self.reset, self.params, self.inertia = reset, params, inertia
        _, values = env_params.redraw_names(self.spec)
        self.values = torch.as_tensor(values, dtype=torch.float64, device=device) if len(values) else None
        self.rspec = env_params.redraw_spec(lib, vcfg, self.spec, self.values.data_ptr() if self.values is not None else None)
        # (an episode's ordinal does not depend on the step count: set_steps means nothing here)
        self.episode_index = torch.zeros(params.shape[1], dtype=torch.int32, device=device)

    def enqueue(self, stream, actions=None):
        native.check(self.lib.vine_env_redraw_scheduled(
            self.handle, self.rspec, self.reset.data_ptr(), self.params.data_ptr(),
            self.inertia.data_ptr() if self.inertia is not None else None, self.episode_index.data_ptr(), stream), self.lib)

    def live_tensors(self):
        """A rolled-back pass has redrawn columns and counted episodes: the tables and the counters go back with the state."""
        return [self.params] + ([self.inertia] if self.inertia is not None else []) + [self.episode_index]

    # -- which plant -------------------------------------------------------------------------------------------------------
    def columns(self, envs, episodes):
        """``draw_columns`` of local env indices ``envs`` in ``episodes``: ``(params [VP_COUNT, M], inertia [VI_COUNT, M] or
        None)``, float32, no device involved."""
        gids = np.asarray(envs, dtype=np.int64) + self.env_id_offset
        return env_params.build_columns(self.spec, self.vcfg, gids, episodes, lib=self.lib, seed=self.seed)
