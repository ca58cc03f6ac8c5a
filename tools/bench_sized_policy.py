"""TOOL: time rollout_batch on board sizes other than 4 with the fused policy off and on (GPU box).

    python tools/bench_sized_policy.py [--lanes 65536] [--max-steps 64] [--repeats 10]
                                       [--out profiles/sized/bench_sized_policy.json]

Per case one agent, one fixed seed list, and in ONE process the two paths of ReinforceAgent.rollout_batch:
  off  the general path (hipBLASLt forward on the obs buffer + g2048_sample + g2048_sized_step per step) -- the code
       every sized rollout ran before g2048_sized_policy existed, untouched: the baseline;
  on   use_fused_sized_policy: g2048_sized_policy + g2048_sized_step per step.
One HIP event pair around each whole rollout (it ends in the rollout's own device synchronisations), 2 warm-up
rollouts per path, then `--repeats` rollouts per path alternating off / on so that both see the same box; median and
p10 / p90 per path, the ratio of the medians, and whether the gap exceeds the two paths' p10-p90 spread.  Before
timing, the two paths' trajectories are compared on the same seeds (lengths and the share of equal actions: the two
forwards differ in the last bits, so a draw within ~1e-6 of a cdf boundary may differ and the episodes then diverge).
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

GENERAL = "hipBLASLt forward (active lanes) + g2048_sample + g2048_sized_step per step"
FUSED = "g2048_sized_policy + g2048_sized_step per step (active lanes)"


def summary(ms: list) -> dict:
    a = np.array(ms)
    return {"median_ms": float(np.median(a)), "p10_ms": float(np.percentile(a, 10)),
            "p90_ms": float(np.percentile(a, 90)), "rollouts": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--max-steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sized", "bench_sized_policy.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sized_policy needs a HIP device: a timing taken elsewhere says nothing")
    from rl2048_amd import Game2048EnvConfig
    from rl2048_amd.agent import ReinforceAgent, ReinforceAgentConfig
    from rl2048_amd.mlp import MLPConfig

    dev = torch.device("cuda", 0)
    n = a.lanes
    es, ps = list(range(n)), list(range(1_000_000, 1_000_000 + n))

    def rollout(agent, on: bool):
        agent.use_fused_sized_policy = on
        b = agent.rollout_batch(es, ps)
        assert agent.last_paths()["rollout"] == (FUSED if on else GENERAL), agent.last_paths()
        return b

    def timed(agent, on: bool) -> float:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        rollout(agent, on)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e)

    out = {"device": torch.cuda.get_device_name(0), "lanes": n, "max_steps": a.max_steps, "cases": []}
    for size in (3, 5, 8):
        for mode, hidden in (("log2", [64, 64]), ("onehot", [256, 128, 64])):
            cfg = Game2048EnvConfig(size=size, obs_mode=mode, obs_log2_scale=0.0625, reward_mode="log2",
                                    base_reward_scale=0.5, max_steps=a.max_steps)
            agent = ReinforceAgent(cfg, MLPConfig(hidden_sizes=hidden, activation="ReLU", init_distribution="HeNormal"),
                                   ReinforceAgentConfig(model_seed=1), device=dev)
            assert agent._sized_spec() is not None
            b0, b1 = rollout(agent, False), rollout(agent, True)          # warm-up 1 + the comparison
            same_len = float((b0.lengths == b1.lengths).float().mean())
            T = min(b0.T, b1.T)
            valid = torch.arange(T, device=dev)[:, None] < torch.minimum(b0.lengths, b1.lengths)[None, :]
            same_act = float((b0.actions[:T] == b1.actions[:T])[valid].float().mean())
            steps = int(b1.lengths.sum())
            del b0, b1
            rollout(agent, False), rollout(agent, True)                   # warm-up 2
            off, on = [], []
            for _ in range(a.repeats):
                off.append(timed(agent, False))
                on.append(timed(agent, True))
            so, sn = summary(off), summary(on)
            spread = (so["p90_ms"] - so["p10_ms"]) + (sn["p90_ms"] - sn["p10_ms"])
            case = {"size": size, "obs": mode, "hidden": hidden, "board_steps": steps, "off": so, "on": sn,
                    "off_over_on": so["median_ms"] / sn["median_ms"],
                    "gap_exceeds_spread": bool(so["median_ms"] - sn["median_ms"] > spread),
                    "episodes_same_length": same_len, "actions_equal_share": same_act}
            out["cases"].append(case)
            print(json.dumps(case), flush=True)
            del agent
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    sys.exit(main())
