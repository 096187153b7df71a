"""Cost of the ENV_TARGET launch (include/vine_env_target.h) behind every step, beside the bare step in the same run: in free
space (the four-lane kernel up to 16384 envs) and in the pipe, each at rest (VEL_ALONG 0 per episode: every lane reads its
flags, its four values and its nine floats of motion state and leaves) and moving (every env at +-0.2 m/s over +-0.05 m: two
observation words and two or three state words more per lane).

Durations come from a replayed hipGraph of K back-to-back (step + launch) pairs between two events (elapsed / K), as
scripts/ubench/env_push_bench.py takes them.  The variants are alternated, ROUNDS times, inside one process.  A moving target
changes the trajectories, so the step of such a run is not the bare run's step bit for bit.

usage: python scripts/ubench/env_target_bench.py [num_envs ...]        (default: 16384)"""
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from env_params_bench import ROUNDS  # noqa: E402
from tests.helpers import base_cfg  # noqa: E402
from tests.hip_env import HipEnv  # noqa: E402
from vine_robot_isaacgymenvs_amd import abi, native  # noqa: E402
from vine_robot_isaacgymenvs_amd.utils import env_target  # noqa: E402

CASES = {"at rest (VEL_ALONG 0, per episode)": {"VEL_ALONG": 0.0, "PER_EPISODE": True},
         "moving (VEL_ALONG +-0.2 over +-0.05)": {"VEL_ALONG": {"values": [0.2, -0.2]}, "SPAN_ALONG": 0.05},
         "moving, redrawn per episode": {"VEL_ALONG": [-0.2, 0.2], "SPAN_ALONG": [0.03, 0.05], "PER_EPISODE": True}}


def make(n, pipe, case):
    cfg = base_cfg(n, 0, True)
    cfg.set_flag(abi.FLAG_CREATE_PIPE, pipe)
    env = type("H", (HipEnv,), {"kernel": None})(cfg)
    env.set_introspection(False)
    tspec = None
    if case is not None:
        spec = env_target.target_config({"ENV_TARGET": CASES[case], "CREATE_PIPE": pipe}, np.float32(cfg.dt) * np.float32(cfg.control_freq_inv))
        _, values = env_target.target_names(spec)
        values_t = torch.as_tensor(values, dtype=torch.float64, device=env.dev) if len(values) else None
        tspec = env_target.target_spec(env.lib, env.cfg, spec, values_t.data_ptr() if len(values) else None)
        table = torch.as_tensor(env_target.draw_target(spec, int(env.cfg.seed), range(n), 0), dtype=torch.float32, device=env.dev).contiguous()
        motion = torch.zeros((abi.VTM_COUNT, n), dtype=torch.float32, device=env.dev)
        fresh = torch.ones(n, dtype=torch.uint8, device=env.dev)
        episode = torch.zeros(n, dtype=torch.int32, device=env.dev)
        env.keep = (tspec, values_t, table, motion, fresh, episode)
    k = 100 if n <= 65536 else 20
    g = torch.Generator(device=env.dev).manual_seed(0)
    acts = [torch.rand((n, 2), device=env.dev, generator=g) * 2 - 1 for _ in range(8)]

    def pair(a):
        env.step_t(a, sync=False)
        if tspec is not None:
            native.check(env.lib.vine_env_target_scheduled(env.h, tspec, env.obs_t.data_ptr(), env.reset_t.data_ptr(), env.progress_t.data_ptr(),
                                                           table.data_ptr(), motion.data_ptr(), fresh.data_ptr(), episode.data_ptr(),
                                                           torch.cuda.current_stream(env.dev).cuda_stream), env.lib)
    for i in range(16):
        pair(acts[i % 8])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        for i in range(k):
            pair(acts[i % 8])
    graph.replay()
    torch.cuda.synchronize()
    return env, graph, k, env.lib.vine_step_kernel_name(env.h).decode()


def main():
    for n in [int(a) for a in sys.argv[1:]] or [16384]:
        for pipe in (False, True):
            envs = {"step alone": make(n, pipe, None)}
            envs.update({"step + target, " + case: make(n, pipe, case) for case in CASES})
            times = {name: [] for name in envs}
            for _ in range(ROUNDS):
                for name, (env, graph, k, _) in envs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    graph.replay()
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1) / k * 1e3)
            print("num_envs %d, %s (%s), %d rounds alternated, one graph replay of %d steps each (us per step: min / median / max)"
                  % (n, "pipe" if pipe else "free space", envs["step alone"][3], ROUNDS, envs["step alone"][2]))
            for name in envs:
                t = times[name]
                print("  %-52s %8.1f %8.1f %8.1f" % (name, min(t), statistics.median(t), max(t)), flush=True)
            base = statistics.median(times["step alone"])
            for case in CASES:
                env = envs["step + target, " + case][0]
                moving = float((env.keep[3][abi.VTM_VEL_ALONG] != 0).float().mean())
                print("  target, %s: %+.2f us per launch (%.1f %% of the envs moving, %.1f %% flagged after the last step; bare run %.1f %%)"
                      % (case, statistics.median(times["step + target, " + case]) - base, 100 * moving,
                         100 * float((env.reset_t != 0).float().mean()), 100 * float((envs["step alone"][0].reset_t != 0).float().mean())))
            for env, _, _, _ in envs.values():
                env.close()
            del envs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
