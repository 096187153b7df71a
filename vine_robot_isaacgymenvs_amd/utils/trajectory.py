"""RECORD_TRAJECTORIES on the host side: the row ring of the step-observer protocol (utils/observers.py) and the MAT files.

The rows are written on the device by ``vine_record_scheduled`` (include/vine_record.h), a launch behind every step that
decides from the device's step counter whether the step just finished belongs to a recording window -- the numeric twin
of CAPTURE_VIDEO (utils/video.py), with the same schedule and the same harvest (``observers.WindowRing``).

One file per recorded env and window, ``<dir>/<time_str>_trajectory_<last>_env<e>.mat``, in the layout ``MAT_FILE``
reads (tasks/vine5link_moving_base.py ``read_mat_file``; V5:281-297) with extra keys beside the reference's six."""
import os

import numpy as np
import torch

from .. import abi, native
from .observers import KEEP, WindowRing  # noqa: F401  (KEEP: importable from here as before)


def record_config(lib, every, steps, num_envs):
    c = abi.VineRecordConfig()
    native.check(lib.vine_record_config_default(c), lib)
    c.record_every, c.num_steps, c.num_envs = int(every), int(steps), int(num_envs)
    return c


def trajectory_arrays(rows, steps, control_dt, env=0, env_params=None, env_param_names=None, env_inertia=None, env_episode=None):
    """The MAT file's variables from the rows of ONE env, ``rows[T, abi.RECORD_FIELDS]`` float32, and the step index of
    every row (with ``env_params``, the env's column of a bound per-env parameter table, also ``env_params`` (VP_COUNT, 1)
    and ``env_param_names``; with ``env_inertia``, the env's column of a bound inertia table, also ``env_inertia``
    (VI_PRIMARY_COUNT, 1): its cart mass, five link masses and five link inertias).  The reference's six keys (V5:281-297) hold positions as (3, T) with a zero x row: the scene is the y-z
    plane.  float32 -> float64 is exact, so a file read back holds the device's values."""
    r = np.asarray(rows)
    assert r.ndim == 2 and r.shape[1] == abi.RECORD_FIELDS, r.shape
    T, f = r.shape[0], abi
    d = r.astype(np.float64).T                       # [F, T]

    def xyz(y, z):
        return np.stack([np.zeros(T), d[y], d[z]])

    extra = {}
    if env_params is not None:                   # ENV_PARAMS: the recorded env's column of the bound table, (VP_COUNT, 1)
        extra = {"env_params": np.asarray(env_params, dtype=np.float64).reshape(-1, 1),
                 "env_param_names": np.array(list(env_param_names), dtype=object)}
    if env_inertia is not None:                  # ENV_INERTIA: the recorded env's 11 primary values
        extra["env_inertia"] = np.asarray(env_inertia, dtype=np.float64).reshape(-1)[:abi.VI_PRIMARY_COUNT].reshape(-1, 1)
    if env_episode is not None:                  # ENV_PARAMS_PER_EPISODE: the ordinal of the env's episode at the harvest, whose
        extra["env_episode"] = np.array([[int(env_episode)]], dtype=np.int64)          # plant env_params / env_inertia hold
    return {
        **extra,
        "cart_pos": d[f.VRF_Q0:f.VRF_Q0 + 1].copy(),
        "Q": d[f.VRF_Q0 + 1:f.VRF_Q0 + abi.NUM_DOFS].copy(),
        "moving_target_pos": xyz(f.VRF_TARGET_Y, f.VRF_TARGET_Z),
        "target_vel": np.zeros((3, 1)),
        "tip_pos": xyz(f.VRF_TIP_Y, f.VRF_TIP_Z),
        "tip_vel": xyz(f.VRF_TIP_VY, f.VRF_TIP_VZ),
        "cart_vel": d[f.VRF_QD0:f.VRF_QD0 + 1].copy(),
        "Qd": d[f.VRF_QD0 + 1:f.VRF_QD0 + abi.NUM_DOFS].copy(),
        "action": d[f.VRF_ACTION0:f.VRF_ACTION0 + abi.NUM_ACTIONS].copy(),
        "smoothed_u_fpam": d[f.VRF_SMOOTHED_U:f.VRF_SMOOTHED_U + 1].copy(),
        "reward": d[f.VRF_REWARD:f.VRF_REWARD + 1].copy(),
        "reset": d[f.VRF_RESET:f.VRF_RESET + 1].copy(),
        "time_out": d[f.VRF_TIMEOUT:f.VRF_TIMEOUT + 1].copy(),
        "progress": d[f.VRF_PROGRESS:f.VRF_PROGRESS + 1].copy(),
        "obj_info": d[f.VRF_OBJ_DEPTH:f.VRF_OBJ_ANGLE + 1].copy(),
        "contact": d[f.VRF_CONTACT:f.VRF_CONTACT + 1].copy(),
        "step": np.asarray(steps, dtype=np.int64).reshape(1, T),
        "dt": np.array([[float(control_dt)]]),
        "env": np.array([[int(env)]], dtype=np.int64),
    }


def write_trajectory_mat(path, rows, steps, control_dt, env=0, env_params=None, env_param_names=None, env_inertia=None,
                         env_episode=None):
    """``trajectory_arrays`` as a MATLAB 5 file at ``path`` (written beside it and renamed: no reader sees half a file)."""
    import scipy.io
    part = path + ".part"
    with open(part, "wb") as fh:
        scipy.io.savemat(fh, trajectory_arrays(rows, steps, control_dt, env, env_params, env_param_names, env_inertia, env_episode))
    os.replace(part, path)
    return path


class TrajectoryRecorder(WindowRing):
    """The row ring of one env handle: a ``WindowRing`` of ``rcfg.num_steps`` rows per recorded env every
    ``rcfg.record_every`` steps."""

    SKIPPED, WRITER = "Trajectories", "trajectory"

    def __init__(self, lib, handle, rcfg, envs, buffers, device, directory, time_str, control_dt, logger=None):
        """``buffers``: the step's output tensors ``(rew, reset, progress, timeouts)``; ``envs``: the K env indices, checked
        by the caller against the env count."""
        self.lib, self.handle, self.rcfg = lib, handle, rcfg
        self.directory, self.time_str, self.control_dt = directory, time_str, float(control_dt)
        self.env_ids = [int(e) for e in envs]
        assert len(self.env_ids) == rcfg.num_envs
        nbytes = int(lib.vine_record_ring_bytes(rcfg))
        if nbytes < 0:
            native.check(nbytes, lib)
        self.envs = torch.as_tensor(self.env_ids, dtype=torch.int32, device=device)
        self.rew, self.reset, self.progress, self.timeouts = buffers
        self.ring = torch.zeros((rcfg.num_steps, rcfg.num_envs, abi.RECORD_FIELDS), dtype=torch.float32, device=device)
        assert self.ring.numel() * 4 == nbytes
        self.steps = torch.full((rcfg.num_steps,), -1, dtype=torch.int64, device=device)
        self.host = torch.empty(self.ring.shape, dtype=torch.float32, pin_memory=True)
        self.host_steps = torch.empty(self.steps.shape, dtype=torch.int64, pin_memory=True)
        self.env_params_of, self.env_param_names = None, None      # ENV_PARAMS: set by the task class when a table is bound
        self.env_inertia_of, self.env_inertia_names = None, None   # ENV_INERTIA: likewise
        self.env_episode_of, self._env_episode = None, None        # ENV_PARAMS_PER_EPISODE: likewise; read at the harvest
        import scipy.io  # noqa: F401  (here, not in the writer thread: the first import takes 0.3 s, longer than a window)
        super().__init__(device, logger)

    def live_tensors(self):
        return [self.ring, self.steps]

    def enqueue(self, stream, actions):
        """The scheduled record, behind the step just enqueued on ``stream`` (captured with it inside a hipGraph)."""
        native.check(self.lib.vine_record_scheduled(self.handle, self.rcfg, self.envs.data_ptr(), actions,
                                                    self.rew.data_ptr(), self.reset.data_ptr(), self.progress.data_ptr(),
                                                    self.timeouts.data_ptr(), self.ring.data_ptr(), self.steps.data_ptr(),
                                                    stream), self.lib)

    def _window(self):
        return self.rcfg.record_every, self.rcfg.num_steps

    def _copies(self):
        return [(self.ring, self.host), (self.steps, self.host_steps)]

    def _job_extra(self):
        self._env_episode = self.env_episode_of(self.env_ids) if self.env_episode_of is not None else None
        return (self.env_params_of(self.env_ids) if self.env_params_of is not None else None,
                self.env_inertia_of(self.env_ids) if self.env_inertia_of is not None else None)

    def path(self, last, env):
        return os.path.join(self.directory, f"{self.time_str}_trajectory_{last}_env{env}.mat")

    def _write(self, start, last, tables):
        params, inertia = tables
        rows, steps = self.host.numpy(), self.host_steps.numpy()
        if not np.array_equal(steps, np.arange(start, last + 1)):       # the device's own account of slot <-> step
            raise RuntimeError(f"window {start}..{last}: the device recorded steps {steps.tolist()}")
        os.makedirs(self.directory, exist_ok=True)
        for k, e in enumerate(self.env_ids):
            self.written.append(write_trajectory_mat(
                self.path(last, e), rows[:, k], steps, self.control_dt, e,
                params[:, k] if params is not None else None, self.env_param_names,
                inertia[:, k] if inertia is not None else None,
                self._env_episode[k] if self._env_episode is not None else None))
        self.logger.info(f"Saved {len(self.env_ids)} trajectories of steps {start}..{last} to "
                         f"{self.path(last, '<e>')}")
