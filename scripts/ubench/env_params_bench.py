"""Duration of the one-lane-per-env step with a per-env parameter table (include/vine_env_params.h), and with the inertia
table beside it (include/vine_env_inertia.h), against the same kernel without one and against the four-lanes-per-env kernel:
free space, default observation layout, randomisation on.

Durations come from a replayed hipGraph of K back-to-back steps between two events (elapsed / K): HIP events around eager
back-to-back launches are host-bound below about 13 us.  The variants are alternated, ROUNDS times, inside one process.

With --redraw: the cost of the per-episode redraw node (include/vine_env_redraw.h) behind every step of the handle with both
heterogeneous tables -- step + node against step alone, the step being the same in each: with no env resetting (the node is
handed a buffer of zeros that no step writes: every lane loads its flag and leaves), with the step's own flags (the task
YAML's episodes under random actions), and with every env resetting every step (a buffer of ones: every lane redraws all
28 + 31 rows).

With --adr: the same three cases for the two launches of ENV_PARAMS_ADR (include/vine_env_adr.h) beside the redraw node in the
same run.  The ADR launches read the reward matrix, and a bound matrix makes the step itself write 52 more bytes per env, so
their baseline is the step alone WITH a matrix bound: node cost = (step + launches) - (that step).

With --draw-adr: --adr, and beside its pair in the same run the two launches of ENV_DRAW_ADR (include/vine_env_draw_adr.h) on the
same handle and against the same baseline: four names under ADR (SENSOR_DELAY, SENSOR_NOISE_STD, PUSH_IMPULSE, TARGET_VEL_ALONG),
the three observers' tables present but their launches not issued, so that the difference is the pair's alone.

With --sensor: the cost of the ENV_SENSOR launch (include/vine_env_sensor.h) behind every step of the default handle (no
table: up to 16384 envs the four-lane kernel), beside the bare step in the same run: idle (delay, hold and noise 0 in every env,
never a first frame: every lane still pushes its frame), with the step's own resets under delays 0..8 and holds, and with
noise on every env (28 Philox calls per env and step).  Reported with the share of the 8 TB/s HBM peak the launch's bytes
over its duration amount to (bytes: the passes over the observation block that case makes).

usage: python scripts/ubench/env_params_bench.py [--redraw | --adr | --draw-adr | --sensor] [num_envs ...]        (default: 16384 1048576)"""
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from tests.helpers import base_cfg  # noqa: E402
from tests.hip_env import HipEnv  # noqa: E402
from vine_robot_isaacgymenvs_amd import abi, native  # noqa: E402
from vine_robot_isaacgymenvs_amd.utils import env_params  # noqa: E402

ROUNDS = 7
SPEC = {"DAMPING": [0.01, 0.05], "SMOOTHING_ALPHA_INFLATE": [0.6, 0.95], "SMOOTHING_ALPHA_DEFLATE": [0.6, 0.95],
        "RAIL_VELOCITY_SCALE": [0.7, 1.3], "RAIL_P_GAIN": [7.0, 13.0], "RAIL_D_GAIN": [0.0, 0.4], "RAIL_ACCELERATION": [5.6, 10.4],
        "ACTION_DELAY": [0, abi.MAX_DELAY], "FPAM_K": [0.8, 1.2], "FPAM_C": [0.8, 1.2], "FPAM_b": [0.8, 1.2], "FPAM_B": [0.8, 1.2]}
MASSES = {"CART_MASS": [0.35, 0.7], "LINK_MASS": [0.7, 1.4], "TIP_LINK_MASS": [0.8, 2.0]}
# name -> (VINE_STEP_KERNEL, table: None / "own" (every column the configuration's row) / "het" (SPEC),
#          inertia table beside it: None / "own" / "het" (MASSES: all 31 rows vary))
VARIANTS = {"lane": ("lane", None, None), "lane+own_row_table": ("lane", "own", None),
            "lane+heterogeneous_table": ("lane", "het", None), "lane+het_table+own_inertia": ("lane", "het", "own"),
            "lane+het_table+het_inertia": ("lane", "het", "het"), "quad": ("quad", None, None)}


ADR_NAMES = {"DAMPING": {"START": [0.03, 0.03], "STEP": 0.005}, "ACTION_DELAY": {"START": [4, 4], "STEP": 1},
             "CART_MASS": {"START": [0.5, 0.5], "STEP": 0.05}, "LINK_MASS": {"START": [1.0, 1.0], "STEP": 0.05},
             "TIP_LINK_MASS": {"START": [1.2, 1.2], "STEP": 0.1}}


def make(n, kern, table, inertia=None, matrix=False, **over):
    cfg = base_cfg(n, 0, True, **over)
    env = type("H", (HipEnv,), {"kernel": kern})(cfg)
    env.set_introspection(False)
    if matrix:
        env.bind_reward_matrix()
    if table is not None:
        t = env_params.build_table(SPEC if table == "het" else {}, env.cfg, 1, n, lib=env.lib)
        env.table_t = torch.as_tensor(t, device=env.dev).contiguous()
        torch.cuda.synchronize()
        native.check(env.lib.vine_bind_env_params(env.h, env.table_t.data_ptr()), env.lib)
    if inertia is not None:
        t = env_params.build_inertia_table(MASSES if inertia == "het" else {"LINK_MASS": 1.0}, env.cfg, 1, n, lib=env.lib)
        env.inertia_t = torch.as_tensor(t, device=env.dev).contiguous()
        torch.cuda.synchronize()
        native.check(env.lib.vine_bind_env_inertia(env.h, env.inertia_t.data_ptr()), env.lib)
    k = 100 if n <= 65536 else 20
    g = torch.Generator(device=env.dev).manual_seed(0)
    acts = [torch.rand((n, 2), device=env.dev, generator=g) * 2 - 1 for _ in range(8)]
    for i in range(16):                                  # episodes under way, kernels loaded
        env.step_t(acts[i % 8], sync=False)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        for i in range(k):
            env.step_t(acts[i % 8], sync=False)
    graph.replay()
    torch.cuda.synchronize()
    return env, graph, k, env.lib.vine_step_kernel_name(env.h).decode()


DRAW_ADR_ENV = {"ENV_SENSOR": {"DELAY": [0, 8], "NOISE_STD": [0.0, 0.02], "PER_EPISODE": True},
                "ENV_PUSH": {"RATE": 0.05, "IMPULSE": [0.0, 0.01], "PER_EPISODE": True},
                "ENV_TARGET": {"VEL_ALONG": [-0.3, 0.3], "SPAN_ALONG": 0.05, "PER_EPISODE": True},
                "ENV_DRAW_ADR": {"NAMES": {"SENSOR_DELAY": {"START": [0, 0], "STEP": 1}, "SENSOR_NOISE_STD": {"START": [0.0, 0.0], "STEP": 0.002},
                                           "PUSH_IMPULSE": {"START": [0.0, 0.0], "STEP": 0.002},
                                           "TARGET_VEL_ALONG": {"START": [0.0, 0.0], "STEP": 0.05}}}}


def draw_adr_node(env, n, flags):
    """The arguments of ``vine_env_draw_adr_scheduled`` on ``env``: the checked spec, the three tables at START, zeroed state."""
    import ctypes as C

    import numpy as np

    from vine_robot_isaacgymenvs_amd.utils import env_draw_adr, env_push, env_sensor, env_target
    cfgs = (env_sensor.sensor_config(DRAW_ADR_ENV, env.num_obs), env_push.push_config(DRAW_ADR_ENV),
            env_target.target_config(DRAW_ADR_ENV, np.float32(env.cfg.dt) * np.float32(env.cfg.control_freq_inv)))
    acfg = env_draw_adr.draw_adr_config(DRAW_ADR_ENV, *cfgs)
    aspec = env_draw_adr.draw_adr_spec(env.lib, env.cfg, acfg, env_sensor.sensor_spec(env.lib, env.cfg, cfgs[0]),
                                       env_push.push_spec(env.lib, env.cfg, cfgs[1]), env_target.target_spec(env.lib, env.cfg, cfgs[2]))
    tables = [torch.zeros((rows, n), device=env.dev) for rows in (abi.VSN_NAMES, abi.VPU_NAMES, abi.VTG_NAMES)]
    i32 = dict(dtype=torch.int32, device=env.dev)
    state = [torch.zeros(18, **i32), torch.zeros(36, **i32), torch.zeros(n, **i32), torch.full((n,), -1, **i32), torch.zeros(n, **i32),
             torch.zeros((acfg["HISTORY_CAPACITY"], 4), **i32), torch.zeros(1, dtype=torch.int64, device=env.dev)]
    pointers = (C.c_void_p * 3)(*[t.data_ptr() for t in tables])
    env.keep_draw_adr = (aspec, tables, state, pointers)
    return [env.h, aspec, flags.data_ptr(), pointers, None] + [t.data_ptr() for t in state]


def make_redraw(n, which, adr=False, draw=False):
    """The handle of ``lane+het_table+het_inertia`` with the redraw node behind every captured step; ``which``: the flags the
    node reads -- "none" (zeros), "own" (the step's reset buffer), "all" (ones).  ``adr``: the two ADR launches in the node's
    place, a reward matrix bound; ``draw``: the two ENV_DRAW_ADR launches in their place."""
    cfg = base_cfg(n, 0, True)
    env = type("H", (HipEnv,), {"kernel": "lane"})(cfg)
    env.set_introspection(False)
    if adr:
        env.bind_reward_matrix()
    spec = dict(SPEC, **MASSES)
    env.table_t = torch.as_tensor(env_params.build_table(spec, env.cfg, 1, n, lib=env.lib), device=env.dev).contiguous()
    env.inertia_t = torch.as_tensor(env_params.build_inertia_table(spec, env.cfg, 1, n, lib=env.lib), device=env.dev).contiguous()
    torch.cuda.synchronize()
    native.check(env.lib.vine_bind_env_params(env.h, env.table_t.data_ptr()), env.lib)
    native.check(env.lib.vine_bind_env_inertia(env.h, env.inertia_t.data_ptr()), env.lib)
    rspec = env_params.redraw_spec(env.lib, env.cfg, spec)
    episode = torch.zeros(n, dtype=torch.int32, device=env.dev)
    flags = {"none": torch.zeros(n, dtype=torch.long, device=env.dev), "own": env.reset_t,
             "all": torch.ones(n, dtype=torch.long, device=env.dev)}[which]
    k = 100 if n <= 65536 else 20
    g = torch.Generator(device=env.dev).manual_seed(0)
    acts = [torch.rand((n, 2), device=env.dev, generator=g) * 2 - 1 for _ in range(8)]

    if adr:
        acfg = env_params.adr_config({"ENV_PARAMS": spec, "ENV_PARAMS_PER_EPISODE": True, "ENV_PARAMS_ADR": {"NAMES": ADR_NAMES}})
        aspec = env_params.adr_spec(env.lib, env.cfg, spec, acfg)
        i32 = dict(dtype=torch.int32, device=env.dev)
        state = [torch.zeros(30, **i32), torch.zeros(60, **i32), torch.zeros(n, **i32), torch.full((n,), -1, **i32),
                 torch.zeros((acfg["HISTORY_CAPACITY"], 4), **i32), torch.zeros(1, dtype=torch.int64, device=env.dev)]
        env.keep_adr = (aspec, state)

    if draw:
        draw_args = draw_adr_node(env, n, flags)

    def pair(a):
        env.step_t(a, sync=False)
        if draw:
            return native.check(env.lib.vine_env_draw_adr_scheduled(*(draw_args + [torch.cuda.current_stream(env.dev).cuda_stream])), env.lib)
        if adr:
            return native.check(env.lib.vine_env_adr_scheduled(
                env.h, aspec, flags.data_ptr(), env.table_t.data_ptr(), env.inertia_t.data_ptr(), episode.data_ptr(),
                *[t.data_ptr() for t in state], torch.cuda.current_stream(env.dev).cuda_stream), env.lib)
        native.check(env.lib.vine_env_redraw_scheduled(env.h, rspec, flags.data_ptr(), env.table_t.data_ptr(), env.inertia_t.data_ptr(),
                                                       episode.data_ptr(), torch.cuda.current_stream(env.dev).cuda_stream), env.lib)
    for i in range(16):
        pair(acts[i % 8])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        for i in range(k):
            pair(acts[i % 8])
    graph.replay()
    torch.cuda.synchronize()
    env.keep = (rspec, episode, flags)
    torch.cuda.synchronize()
    env.reset_share = float((env.reset_t != 0).float().mean())
    return env, graph, k, env.lib.vine_step_kernel_name(env.h).decode() + (" + draw adr" if draw else " + adr" if adr else " + redraw")


def main_redraw(sizes, adr=False, draw=False):
    for n in sizes:
        envs = {"step alone (both het tables)": make(n, "lane", "het", "het"),
                "step + node, no env resetting": make_redraw(n, "none"),
                "step + node, the step's own resets": make_redraw(n, "own"),
                "step + node, every env resetting": make_redraw(n, "all")}
        if adr:
            envs.update({"step alone, reward matrix bound": make(n, "lane", "het", "het", matrix=True),
                         "step + adr, no env resetting": make_redraw(n, "none", True),
                         "step + adr, the step's own resets": make_redraw(n, "own", True),
                         "step + adr, every env resetting": make_redraw(n, "all", True)})
        if draw:
            envs.update({"step + draw adr, no env resetting": make_redraw(n, "none", True, True),
                         "step + draw adr, the step's own resets": make_redraw(n, "own", True, True),
                         "step + draw adr, every env resetting": make_redraw(n, "all", True, True)})
        times = {name: [] for name in envs}
        for _ in range(ROUNDS):
            for name, (env, graph, k, _) in envs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graph.replay()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / k * 1e3)
        print("num_envs %d, %d rounds alternated, one graph replay of %d steps each (us per step: min / median / max)"
              % (n, ROUNDS, next(iter(envs.values()))[2]))
        for name in envs:
            t = times[name]
            print("  %-36s %8.1f %8.1f %8.1f" % (name, min(t), statistics.median(t), max(t)), flush=True)
        base = statistics.median(times["step alone (both het tables)"])
        for name in list(envs)[1:4]:
            own = " (%.1f %% of the envs flagged after the last step)" % (100 * envs[name][0].reset_share) if "own" in name else ""
            print("  node, %s: %+.2f us per launch%s" % (name.split(", ")[1], statistics.median(times[name]) - base, own))
        if adr:
            base = statistics.median(times["step alone, reward matrix bound"])
            for name in list(envs)[5:]:
                own = " (%.1f %% of the envs flagged after the last step)" % (100 * envs[name][0].reset_share) if "own" in name else ""
                print("  %s launches, %s: %+.2f us per pair%s" % ("draw adr" if "draw adr" in name else "adr", name.split(", ")[1],
                                                                 statistics.median(times[name]) - base, own))
        for env, _, _, _ in envs.values():
            env.close()
        del envs
        torch.cuda.empty_cache()


SENSOR_CASES = {  # name -> (ENV_SENSOR keys, the progress the launch reads: "busy" = never 0, "own" = the step's, passes)
    "idle": ({"DELAY": 0, "PER_EPISODE": True}, "busy", 2),                                        # read the buffer, write a slot
    "the step's own resets": ({"DELAY": [0, 8], "HOLD": [0.0, 0.3], "PER_EPISODE": True}, "own", 4),
    "noise on every env": ({"DELAY": [0, 8], "NOISE_STD": 0.01, "PER_EPISODE": True}, "own", 4)}
HBM_PEAK = 8.0e12


def make_sensor(n, case):
    from vine_robot_isaacgymenvs_amd.utils import env_sensor
    keys, which, _ = SENSOR_CASES[case]
    cfg = base_cfg(n, 0, True)
    env = type("H", (HipEnv,), {"kernel": None})(cfg)
    env.set_introspection(False)
    spec = env_sensor.sensor_config({"ENV_SENSOR": keys}, env.num_obs)
    sspec = env_sensor.sensor_spec(env.lib, env.cfg, spec)
    table = torch.as_tensor(env_sensor.draw_sensor(spec, int(env.cfg.seed), range(n), 0), dtype=torch.float32, device=env.dev).contiguous()
    ring = torch.zeros((abi.SENSOR_SLOTS, n, env.num_obs), device=env.dev)
    fresh = torch.ones(n, dtype=torch.uint8, device=env.dev)
    episode = torch.zeros(n, dtype=torch.int32, device=env.dev)
    progress = env.progress_t if which == "own" else torch.ones(n, dtype=torch.long, device=env.dev)
    k = 100 if n <= 65536 else 20
    g = torch.Generator(device=env.dev).manual_seed(0)
    acts = [torch.rand((n, 2), device=env.dev, generator=g) * 2 - 1 for _ in range(8)]

    def pair(a):
        env.step_t(a, sync=False)
        native.check(env.lib.vine_env_sensor_scheduled(env.h, sspec, env.obs_t.data_ptr(), env.reset_t.data_ptr(), progress.data_ptr(),
                                                       table.data_ptr(), ring.data_ptr(), fresh.data_ptr(), episode.data_ptr(),
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
    env.keep = (sspec, table, ring, fresh, episode, progress)
    return env, graph, k, env.lib.vine_step_kernel_name(env.h).decode() + " + sensor"


def main_sensor(sizes):
    for n in sizes:
        envs = {"step alone": make(n, None, None)}
        envs.update({"step + sensor, " + case: make_sensor(n, case) for case in SENSOR_CASES})
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
            print("  %-40s %8.1f %8.1f %8.1f" % (name, min(t), statistics.median(t), max(t)), flush=True)
        base = statistics.median(times["step alone"])
        block = n * envs["step alone"][0].num_obs * 4
        for case, (_, _, passes) in SENSOR_CASES.items():
            cost = statistics.median(times["step + sensor, " + case]) - base
            share = passes * block / (cost * 1e-6) / HBM_PEAK if cost > 0 else float("nan")
            print("  sensor, %s: %+.2f us per launch; %d passes over the %.2f MB observation block = %.1f %% of the HBM peak"
                  % (case, cost, passes, block / 1e6, 100 * share))
        for env, _, _, _ in envs.values():
            env.close()
        del envs
        torch.cuda.empty_cache()


def main():
    if "--sensor" in sys.argv[1:]:
        return main_sensor([int(a) for a in sys.argv[1:] if a != "--sensor"] or [16384, 1 << 20])
    args = [a for a in sys.argv[1:] if a not in ("--redraw", "--adr", "--draw-adr")]
    if "--redraw" in sys.argv[1:] or "--adr" in sys.argv[1:] or "--draw-adr" in sys.argv[1:]:
        draw = "--draw-adr" in sys.argv[1:]
        return main_redraw([int(a) for a in args] or [16384, 1 << 20], adr=draw or "--adr" in sys.argv[1:], draw=draw)
    for n in [int(a) for a in args] or [16384, 1 << 20]:
        envs = {name: make(n, *v) for name, v in VARIANTS.items()}
        times = {name: [] for name in VARIANTS}
        for _ in range(ROUNDS):
            for name, (env, graph, k, _) in envs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graph.replay()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / k * 1e3)
        print("num_envs %d, %d rounds alternated, one graph replay of %d steps each (us per step: min / median / max)"
              % (n, ROUNDS, envs["lane"][2]))
        for name in VARIANTS:
            t = times[name]
            print("  %-28s %-22s %8.1f %8.1f %8.1f" % (name, envs[name][3], min(t), statistics.median(t), max(t)), flush=True)
        base, het, quad = (statistics.median(times[k]) for k in ("lane", "lane+heterogeneous_table", "quad"))
        print("  heterogeneous table / unbound one-lane: %.3f   / four-lane: %.3f" % (het / base, het / quad))
        mass = statistics.median(times["lane+het_table+het_inertia"])
        print("  heterogeneous table and inertia table / heterogeneous table: %.3f   / unbound one-lane: %.3f" % (mass / het, mass / base))
        for env, _, _, _ in envs.values():
            env.close()
        del envs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
