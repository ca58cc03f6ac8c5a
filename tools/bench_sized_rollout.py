"""TOOL: time rollout_batch on board sizes other than 4 on its three paths (GPU box).

    python tools/bench_sized_rollout.py [--lanes 65536] [--max-steps 64] [--repeats 10]
                                        [--out profiles/sized/bench_sized_rollout.json]

The protocol of tools/bench_sized_policy.py with a third path.  Per case one agent, one fixed seed list, and in ONE
process the three paths of ReinforceAgent.rollout_batch:
  general     hipBLASLt forward on the obs buffer + g2048_sample + g2048_sized_step per step (the default);
  policy      use_fused_sized_policy: g2048_sized_policy + g2048_sized_step per step;
  persistent  use_fused_sized_rollout: g2048_sized_rollout, the whole rollout in persistent launches.
One HIP event pair around each whole rollout (it ends in the rollout's own device synchronisations), 2 warm-up
rollouts per path, then `--repeats` rollouts per path alternating general / policy / persistent so that all see the
same box; median and p10 / p90 per path.  The claim under test: persistent beats policy by more than the two paths'
p10-p90 spreads together (`beats_policy_by_more_than_spread`); the table is reported as measured either way.  Before
timing, the paths' trajectories are compared on the same seeds: persistent and policy run the same forward, choice
and env step, so their lengths and actions must be equal; the general path's forward differs in the last bits, so
its share of equal actions is reported (a draw within ~1e-6 of a cdf boundary may differ, and the episode then
diverges).
Cases: N in {3, 5, 8} x {log2 [64, 64], one-hot [256, 128, 64]}, ReLU.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATHS = {"general": "hipBLASLt forward (active lanes) + g2048_sample + g2048_sized_step per step",
         "policy": "g2048_sized_policy + g2048_sized_step per step (active lanes)",
         "persistent": "g2048_sized_rollout (persistent launches, suspended episodes resumed)"}


def summary(ms: list) -> dict:
    a = np.array(ms)
    return {"median_ms": float(np.median(a)), "p10_ms": float(np.percentile(a, 10)),
            "p90_ms": float(np.percentile(a, 90)), "rollouts": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--max-steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sized", "bench_sized_rollout.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sized_rollout needs a HIP device: a timing taken elsewhere says nothing")
    from rl2048_amd import Game2048EnvConfig
    from rl2048_amd.agent import ReinforceAgent, ReinforceAgentConfig
    from rl2048_amd.mlp import MLPConfig

    dev = torch.device("cuda", 0)
    n = a.lanes
    es, ps = list(range(n)), list(range(1_000_000, 1_000_000 + n))

    def rollout(agent, path: str):
        agent.use_fused_sized_policy = path == "policy"
        agent.use_fused_sized_rollout = path == "persistent"
        b = agent.rollout_batch(es, ps)
        assert agent.last_paths()["rollout"] == PATHS[path], agent.last_paths()
        return b

    def timed(agent, path: str) -> float:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        rollout(agent, path)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e)

    def same(b0, b1):
        T = min(b0.T, b1.T)
        valid = torch.arange(T, device=dev)[:, None] < torch.minimum(b0.lengths, b1.lengths)[None, :]
        return (float((b0.lengths == b1.lengths).float().mean()),
                float((b0.actions[:T] == b1.actions[:T])[valid].float().mean()))

    out = {"device": torch.cuda.get_device_name(0), "lanes": n, "max_steps": a.max_steps, "cases": []}
    for size in (3, 5, 8):
        for mode, hidden in (("log2", [64, 64]), ("onehot", [256, 128, 64])):
            cfg = Game2048EnvConfig(size=size, obs_mode=mode, obs_log2_scale=0.0625, reward_mode="log2",
                                    base_reward_scale=0.5, max_steps=a.max_steps)
            agent = ReinforceAgent(cfg, MLPConfig(hidden_sizes=hidden, activation="ReLU", init_distribution="HeNormal"),
                                   ReinforceAgentConfig(model_seed=1), device=dev)
            assert agent._sized_spec() is not None
            bg, bp, br = (rollout(agent, p) for p in PATHS)               # warm-up 1 + the comparison
            pol_len, pol_act = same(bp, br)
            gen_len, gen_act = same(bg, br)
            assert pol_len == 1.0 and pol_act == 1.0, "persistent and policy paths must play the same episodes"
            steps = int(br.lengths.sum())
            del bg, bp, br
            for p in PATHS:                                               # warm-up 2
                rollout(agent, p)
            ms = {p: [] for p in PATHS}
            for _ in range(a.repeats):
                for p in PATHS:
                    ms[p].append(timed(agent, p))
            s = {p: summary(v) for p, v in ms.items()}
            spread = (s["policy"]["p90_ms"] - s["policy"]["p10_ms"]) + (s["persistent"]["p90_ms"] - s["persistent"]["p10_ms"])
            case = {"size": size, "obs": mode, "hidden": hidden, "board_steps": steps, **s,
                    "policy_over_persistent": s["policy"]["median_ms"] / s["persistent"]["median_ms"],
                    "general_over_persistent": s["general"]["median_ms"] / s["persistent"]["median_ms"],
                    "beats_policy_by_more_than_spread":
                        bool(s["policy"]["median_ms"] - s["persistent"]["median_ms"] > spread),
                    "policy_vs_persistent": {"episodes_same_length": pol_len, "actions_equal_share": pol_act},
                    "general_vs_persistent": {"episodes_same_length": gen_len, "actions_equal_share": gen_act}}
            out["cases"].append(case)
            print(json.dumps(case), flush=True)
            del agent
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    sys.exit(main())
