"""Cost of the ENV_PUSH launch (include/vine_env_push.h) behind every step of the default handle (no table: up to 16384 envs
the four-lane kernel), beside the bare step in the same run: idle (RATE 1e-9 in every env: every lane reads its reset word
and its two values, makes its Philox call and leaves) and with RATE 0.05, IMPULSE 0.005 on every env (one lane in twenty
loads its eleven state words, factors its mass matrix and stores six velocities; the others wait for it in their wave).

Durations come from a replayed hipGraph of K back-to-back (step + launch) pairs between two events (elapsed / K), as
scripts/ubench/env_params_bench.py takes them.  The variants are alternated, ROUNDS times, inside one process.  Pushes change
the trajectories, so the step of a pushed run is not the bare run's step bit for bit; at RATE 0.05 the share of envs that
reset does not move visibly (printed).

usage: python scripts/ubench/env_push_bench.py [num_envs ...]        (default: 16384 1048576)"""
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from env_params_bench import ROUNDS, make  # noqa: E402
from tests.helpers import base_cfg  # noqa: E402
from tests.hip_env import HipEnv  # noqa: E402
from vine_robot_isaacgymenvs_amd import native  # noqa: E402
from vine_robot_isaacgymenvs_amd.utils import env_push  # noqa: E402

CASES = {"idle (RATE 1e-9)": {"RATE": 1e-9, "IMPULSE": 0.005},
         "RATE 0.05 on every env": {"RATE": 0.05, "IMPULSE": 0.005},
         "RATE 0.05, points [0, 2, 5]": {"RATE": 0.05, "IMPULSE": [0.0, 0.01], "POINTS": [0, 2, 5], "PER_EPISODE": True}}


def make_push(n, case):
    cfg = base_cfg(n, 0, True)
    env = type("H", (HipEnv,), {"kernel": None})(cfg)
    env.set_introspection(False)
    spec = env_push.push_config({"ENV_PUSH": CASES[case]})
    pspec = env_push.push_spec(env.lib, env.cfg, spec)
    table = torch.as_tensor(env_push.draw_push(spec, int(env.cfg.seed), range(n), 0), dtype=torch.float32, device=env.dev).contiguous()
    episode = torch.zeros(n, dtype=torch.int32, device=env.dev)
    count = torch.zeros(n, dtype=torch.int32, device=env.dev)
    k = 100 if n <= 65536 else 20
    g = torch.Generator(device=env.dev).manual_seed(0)
    acts = [torch.rand((n, 2), device=env.dev, generator=g) * 2 - 1 for _ in range(8)]

    def pair(a):
        env.step_t(a, sync=False)
        native.check(env.lib.vine_env_push_scheduled(env.h, pspec, env.reset_t.data_ptr(), table.data_ptr(), episode.data_ptr(),
                                                     count.data_ptr(), torch.cuda.current_stream(env.dev).cuda_stream), env.lib)
    for i in range(16):
        pair(acts[i % 8])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        for i in range(k):
            pair(acts[i % 8])
    graph.replay()
    torch.cuda.synchronize()
    env.keep = (pspec, table, episode, count)
    return env, graph, k, env.lib.vine_step_kernel_name(env.h).decode() + " + push"


def main():
    for n in [int(a) for a in sys.argv[1:]] or [16384, 1 << 20]:
        envs = {"step alone": make(n, None, None)}
        envs.update({"step + push, " + case: make_push(n, case) for case in CASES})
        times = {name: [] for name in envs}
        for _ in range(ROUNDS):
            for name, (env, graph, k, _) in envs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graph.replay()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / k * 1e3)
        print("num_envs %d (%s), %d rounds alternated, one graph replay of %d steps each (us per step: min / median / max)"
              % (n, envs["step alone"][3], ROUNDS, envs["step alone"][2]))
        for name in envs:
            t = times[name]
            print("  %-44s %8.1f %8.1f %8.1f" % (name, min(t), statistics.median(t), max(t)), flush=True)
        base = statistics.median(times["step alone"])
        for case in CASES:
            env = envs["step + push, " + case][0]
            pushes = int(env.keep[3].sum())
            print("  push, %s: %+.2f us per launch (%.2f %% of the envs pushed per step, %.1f %% flagged after the last step; bare run %.1f %%)"
                  % (case, statistics.median(times["step + push, " + case]) - base, 100.0 * pushes / (n * int(env.step_count)),
                     100 * float((env.reset_t != 0).float().mean()), 100 * float((envs["step alone"][0].reset_t != 0).float().mean())))
        for env, _, _, _ in envs.values():
            env.close()
        del envs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
