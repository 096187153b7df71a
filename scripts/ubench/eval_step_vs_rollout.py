"""vine_step_eval against vine_step_rollout on the same workload: twin envs (same seed), the same LSTM output rows and head, and
logstd = -20 so that the rollout's sampled action is its mean to 2e-9 -- the two envs then walk the same trajectory and the
two kernels see the same contacts.  (A player run and a training run do not: the policies act differently and the pipe
configuration's step time follows the contacts.)  HIP events around blocks of 100 launches, alternated; run it under
`rocprofv3 --kernel-trace --stats` for the per-kernel durations.

  python scripts/ubench/eval_step_vs_rollout.py [--envs 16384] [--blocks 6]
"""
import argparse
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from vine_robot_isaacgymenvs_amd import abi, load_config  # noqa: E402
from vine_robot_isaacgymenvs_amd.learning import fused  # noqa: E402
from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map  # noqa: E402

H, A = 256, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--blocks", type=int, default=6)
    args = ap.parse_args()
    N, dev, lib = args.envs, torch.device("cuda:0"), fused._lib()
    st = torch.cuda.current_stream().cuda_stream
    for name, ov in (("free", ["task.env.CREATE_PIPE=False"]), ("pipe", [])):
        def make():
            cfg = load_config(overrides=["num_envs=%d" % N] + ov)
            cfg["task"]["seed"] = 42
            return isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg["task"], rl_device="cuda:0", sim_device="cuda:0",
                                                          graphics_device_id=0, headless=True)
        er, ee = make(), make()
        g = torch.Generator(device=dev).manual_seed(1)
        rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
        gamma, beta = 1.0 + 0.1 * rnd(H), 0.1 * rnd(H)
        w_mu, b_mu, w_v, b_v = 0.05 * rnd(A, H), 0.1 * rnd(A), 0.1 * rnd(1, H), 0.1 * rnd(1)
        logstd = torch.full((2,), -20.0, device=dev)
        hw, hc = torch.empty(3 * H, device=dev), torch.empty(3, device=dev)
        fused._check(lib.vine_rollout_head_prep(gamma.data_ptr(), beta.data_ptr(), w_mu.data_ptr(), b_mu.data_ptr(), w_v.data_ptr(),
                                                b_v.data_ptr(), hw.data_ptr(), hc.data_ptr(), st), "head_prep")
        ys = [rnd(N, H) for _ in range(8)]
        counter = torch.zeros(1, device=dev, dtype=torch.int64)
        vmean, vvar = torch.zeros(1, device=dev, dtype=torch.float64), torch.ones(1, device=dev, dtype=torch.float64)
        f32 = lambda *s: torch.zeros(*s, device=dev)
        u8 = lambda *s: torch.zeros(*s, device=dev, dtype=torch.uint8)
        r = dict(mu=f32(N, A), sigma=f32(N, A), value=f32(N), action=f32(N, A), nlp=f32(N), shaped=f32(N), dones=u8(N), cur_r=f32(N),
                 cur_l=f32(N), h=f32(N, H), c=f32(N, H), hop=f32(N, 352), partial=f32(abi.ROLLOUT_POST_SCRATCH_FLOATS), obs=f32(N, er.num_obs))
        e = dict(mu=f32(N, A), action=f32(N, A), dones=u8(N), h=f32(N, H), c=f32(N, H), hop=f32(N, 352), obs=f32(N, ee.num_obs),
                 episode=f32(abi.EVAL_EPISODE_FIELDS, N), totals=torch.zeros(ee.eval_step_rows(), abi.EVAL_NUM_TOTALS, device=dev, dtype=torch.float64))
        e["episode"][abi.EVAL_EP_MIN_DIST] = math.inf

        def roll(y):
            a = abi.RolloutArgs()
            a.y, a.hw, a.hc, a.logstd = y.data_ptr(), hw.data_ptr(), hc.data_ptr(), logstd.data_ptr()
            a.value_mean, a.value_var, a.ln_eps, a.value_eps = vmean.data_ptr(), vvar.data_ptr(), 1e-5, 1e-5
            a.seed, a.counter = 12345, counter.data_ptr()
            a.mu_out, a.sigma_out, a.value_out = r["mu"].data_ptr(), r["sigma"].data_ptr(), r["value"].data_ptr()
            a.action_out, a.neglogp_out = r["action"].data_ptr(), r["nlp"].data_ptr()
            a.reward_shift, a.reward_scale, a.gamma_bootstrap = 0.0, 0.01, 0.99
            a.shaped_out, a.dones_out, a.cur_rewards, a.cur_lengths = r["shaped"].data_ptr(), r["dones"].data_ptr(), r["cur_r"].data_ptr(), r["cur_l"].data_ptr()
            a.h_state, a.c_state, a.h_op, a.h_op_stride = r["h"].data_ptr(), r["c"].data_ptr(), r["hop"].data_ptr() + 4 * 96, 352
            a.partial = r["partial"].data_ptr()
            er.step_rollout_into(a, r["obs"])

        def ev(y):
            a = abi.EvalArgs()
            a.y, a.hw, a.hc, a.logstd = y.data_ptr(), hw.data_ptr(), hc.data_ptr(), logstd.data_ptr()
            a.ln_eps, a.deterministic, a.seed = 1e-5, 1, 12345
            a.mu_out, a.action_out, a.dones_out = e["mu"].data_ptr(), e["action"].data_ptr(), e["dones"].data_ptr()
            a.h_state, a.c_state, a.h_op, a.h_op_stride = e["h"].data_ptr(), e["c"].data_ptr(), e["hop"].data_ptr() + 4 * 96, 352
            a.episode, a.totals = e["episode"].data_ptr(), e["totals"].data_ptr()
            ee.step_eval_into(a, e["obs"])

        for blk in range(args.blocks):
            for label, fn in (("rollout", roll), ("eval", ev)):
                s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for i in range(100):
                    fn(ys[i % 8])
                t.record()
                torch.cuda.synchronize()
                print("%s block %d %-7s %.2f us per launch" % (name, blk, label, s.elapsed_time(t) * 10), flush=True)
        same = float((r["obs"] - e["obs"]).abs().max())
        print("%s: max |obs diff| between the twins after %d steps %.3e; episodes %d" % (name, 100 * args.blocks, same, int(e["totals"][:, 0].sum())))
        er.close(); ee.close()


if __name__ == "__main__":
    main()
