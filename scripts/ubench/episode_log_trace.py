"""A workload for a rocprofv3 kernel trace of the EPISODE_LOG launch, and the summary of that trace.

  rocprofv3 --kernel-trace --output-format csv -d <dir> -- python scripts/ubench/episode_log_trace.py run <counts.json> [idle|busy]
  python scripts/ubench/episode_log_trace.py summarise <dir> <counts.json>

``run``: 16384 envs, free space, 64 ``VecTask.step`` calls with the log on.  ``idle``: the task's 500-step episodes and zero
actions, so that no episode ends; ``busy``: 12-step episodes and random actions.  After every step the cursor is read
(the trace is of kernels, the host's pace does not matter) and the number of rows each launch appended is written to
``counts.json``.  ``summarise`` pairs launch i of vine_episodes_kernel with that count."""
import csv
import glob
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)


def run(out, mode, n=16384, steps=64):
    import tempfile
    import torch
    from vine_robot_isaacgymenvs_amd import load_task_config
    from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=%d" % n])
    cfg["seed"] = 42
    cfg["env"].update(CREATE_PIPE=False, EPISODE_LOG=True, EPISODE_LOG_DIR=tempfile.mkdtemp(prefix="vine_episodes_"))
    if mode == "busy":
        cfg["env"].update(maxEpisodeLength=12)
    env = isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg, rl_device="cuda:0", sim_device="cuda:0", graphics_device_id=0,
                                                    headless=True)
    g = torch.Generator(device=env.device).manual_seed(1)
    counts, last = [], 0
    for _ in range(steps):
        a = torch.zeros((n, 2), device=env.device)
        if mode == "busy":
            a = torch.rand((n, 2), device=env.device, generator=g) * 2 - 1
        env.step(a)
        cursor = int(env.episode_log.cursor.item())
        counts.append(cursor - last)
        last = cursor
    json.dump({"mode": mode, "envs": n, "rows_per_launch": counts}, open(out, "w"))
    env.close()


def summarise(directory, counts_file):
    counts = json.load(open(counts_file))
    f = glob.glob(os.path.join(directory, "*", "*_kernel_trace.csv"))[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3      # noqa: E731
    mine = [us(r) for r in rows if "vine_episodes_kernel" in r["Kernel_Name"]]
    step = [us(r) for r in rows if "vine_step" in r["Kernel_Name"]]
    per = counts["rows_per_launch"]
    print("%s: %d envs, episode kernel launches %d (step kernel launches %d, median %.2f us)"
          % (counts["mode"], counts["envs"], len(mine), len(step), statistics.median(step)))
    assert len(mine) == len(per)
    for label, sel in (("idle (no row)", [d for d, c in zip(mine, per) if c == 0]),
                       ("with finished episodes", [d for d, c in zip(mine, per) if c > 0])):
        if sel:
            print("  %s: %d launches, min %.2f median %.2f max %.2f us" % (label, len(sel), min(sel), statistics.median(sel), max(sel)))
    print("  rows per launch:", " ".join(str(c) for c in per))
    print("  durations us:", " ".join("%.2f" % d for d in mine))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else "idle")
    else:
        summarise(sys.argv[2], sys.argv[3])
