"""TOOL: time and weigh evaluation through rollout_batch against the score-only evaluate_batch (GPU box).

    python tools/bench_eval.py [--episodes 65536] [--repeats 5] [--out profiles/eval/bench_eval.json]

Two cases, `--episodes` episodes each, greedy as an evaluation is, max_steps None:
  runner   4 x 4, one-hot [256, 128, 64] ReLU (the runner config's net): g2048_deep_rollout / g2048_deep_eval;
  sized    N = 5, log2 [64, 64] ReLU, use_fused_sized_rollout on: g2048_sized_rollout / g2048_sized_eval.
Per case one agent and one fixed seed list, and in ONE process the two paths
  trajectory   ReinforceAgent.rollout_batch (the whole time-major trajectory is materialised);
  score_only   ReinforceAgent.evaluate_batch (the same kernels without the trajectory row).
One warm-up call per path, whose per-episode results are compared bit for bit (the paths play the same episodes), then
`--repeats` calls per path alternating trajectory / score_only so that both see the same box.  Per call: wall time
(host clock around the call and a device synchronisation) and torch.cuda.max_memory_allocated with the peak reset
before the call, also as the increase over what was allocated before it.  The file holds every call's figures, so the
trajectory path's own run-to-run spread (at least three calls) stands beside the difference between the paths.  No
speed-up is claimed: the time is a report.  What the score-only path is for is the memory column.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"runner": dict(size=4, obs_mode="onehot", hidden=[256, 128, 64], sized_switch=False),
         "sized": dict(size=5, obs_mode="log2", hidden=[64, 64], sized_switch=True)}


def summary(calls: list) -> dict:
    t = np.array([c["wall_s"] for c in calls])
    return {"median_s": float(np.median(t)), "min_s": float(t.min()), "max_s": float(t.max()),
            "peak_allocated_bytes": int(max(c["peak_allocated_bytes"] for c in calls)),
            "peak_increase_bytes": int(max(c["peak_increase_bytes"] for c in calls)), "calls": calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval", "bench_eval.json"))
    a = ap.parse_args()
    if a.repeats < 3:
        sys.exit("--repeats must be at least 3: the trajectory path's own spread belongs in the file")
    if not torch.cuda.is_available():
        sys.exit("bench_eval needs a HIP device: a timing taken elsewhere says nothing")
    from rl2048_amd import Game2048EnvConfig
    from rl2048_amd.agent import ReinforceAgent, ReinforceAgentConfig
    from rl2048_amd.mlp import MLPConfig

    dev = torch.device("cuda", 0)
    n = a.episodes
    es = np.arange(n, dtype=np.int64)
    ps = es + 1_000_000

    def play(agent, path: str):
        if path == "trajectory":
            return agent.rollout_batch(es, ps, use_greedy=True)
        return agent.evaluate_batch(es, ps, use_greedy=True)

    def measured(agent, path: str) -> dict:
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        t0 = time.perf_counter()
        b = play(agent, path)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        peak = torch.cuda.max_memory_allocated(dev)
        del b
        return {"wall_s": wall, "peak_allocated_bytes": int(peak), "peak_increase_bytes": int(peak - base)}

    out = {"device": torch.cuda.get_device_name(0), "episodes": n, "repeats": a.repeats, "cases": {}}
    for name, c in CASES.items():
        cfg = Game2048EnvConfig(size=c["size"], obs_mode=c["obs_mode"], obs_log2_scale=0.0625, reward_mode="log2",
                                base_reward_scale=0.5, use_action_mask=True, max_steps=None)
        agent = ReinforceAgent(cfg, MLPConfig(hidden_sizes=c["hidden"], activation="ReLU", init_distribution="HeNormal"),
                               ReinforceAgentConfig(model_seed=1), device=dev)
        agent.use_fused_sized_rollout = c["sized_switch"]
        tb, ev = play(agent, "trajectory"), play(agent, "score_only")          # warm-up + the comparison
        paths = {"trajectory": agent.last_paths()["rollout"], "score_only": agent.last_paths()["eval"]}
        assert "_rollout (persistent" in paths["trajectory"] and "_eval (persistent" in paths["score_only"], paths
        same = all(torch.equal(getattr(tb, f), getattr(ev, f)) for f in ("lengths", "max_tile", "final_boards")) and \
            torch.equal(tb.total_reward.view(torch.int64), ev.total_reward.view(torch.int64))
        assert same, "the two paths must play the same episodes"
        steps, longest = int(tb.lengths.sum()), int(tb.lengths.max())
        del tb, ev
        calls = {"trajectory": [], "score_only": []}
        for _ in range(a.repeats):
            for p in calls:
                calls[p].append(measured(agent, p))
        s = {p: summary(v) for p, v in calls.items()}
        spread = s["trajectory"]["max_s"] - s["trajectory"]["min_s"]
        case = {"size": c["size"], "obs": c["obs_mode"], "hidden": c["hidden"], "paths": paths, "board_steps": steps,
                "longest_episode": longest, "same_episodes": same, **s,
                "trajectory_spread_s": spread,
                "score_only_minus_trajectory_s": s["score_only"]["median_s"] - s["trajectory"]["median_s"],
                "score_only_slower_by_more_than_trajectory_spread":
                    bool(s["score_only"]["median_s"] - s["trajectory"]["median_s"] > spread),
                "peak_increase_ratio": s["trajectory"]["peak_increase_bytes"] / max(s["score_only"]["peak_increase_bytes"], 1)}
        out["cases"][name] = case
        print(json.dumps({k: v for k, v in case.items() if k not in calls}
                         | {p: {k: v for k, v in s[p].items() if k != "calls"} for p in calls}), flush=True)
        del agent
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    sys.exit(main())
