"""TOOL: time update_from_batch on board sizes other than 4 on its two gradient paths (GPU box).

    python tools/bench_sized_grad.py [--lanes 65536] [--max-steps 64] [--repeats 10]
                                     [--out profiles/sized/bench_sized_grad.json]

The protocol of tools/bench_sized_rollout.py.  Per case one actor-critic agent and ONE rollout of `--lanes` episodes
(the persistent rollout kernel: it only supplies the batch), then in ONE process the two paths of the update:
  general  g2048_sized_obs rows + hipBLASLt forward + torch backward ("hipBLASLt backprop", the default);
  fused    use_fused_sized_grad: g2048_sized_grad (+ g2048_sized_onehot_dw1 on one-hot obs) per chunk.
update_from_batch alone is timed, one HIP event pair per call, on copies of the parameters (SGD: no optimiser state)
restored before every call (so every call sees the same weights and the same ReLU pattern); 2 warm-up calls per path,
then `--repeats` per path with the switch alternating off / on so that both see the same box; median and p10 / p90
per path.  The claim under test: fused beats general by more than the two paths' p10-p90 spreads together
(`beats_general_by_more_than_spread`); the table is reported as measured either way.  Before timing, the two paths'
pre-clip gradients are compared (`max_normwise_gradient_difference`: the largest, over all tensors, of
max |fused - general| / max |general|, the convention of tests/exact_grad.py's _rel).
Cases: N in {3, 5, 8} x {log2 [64, 64], one-hot [256, 128, 64]}, ReLU, actor-critic (MSE).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GENERAL = "hipBLASLt backprop"


def summary(ms: list) -> dict:
    a = np.array(ms)
    return {"median_ms": float(np.median(a)), "p10_ms": float(np.percentile(a, 10)),
            "p90_ms": float(np.percentile(a, 90)), "updates": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--max-steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sized", "bench_sized_grad.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sized_grad needs a HIP device: a timing taken elsewhere says nothing")
    from rl2048_amd import Game2048EnvConfig
    from rl2048_amd.agent import ReinforceAgent, ReinforceAgentConfig
    from rl2048_amd.mlp import MLPConfig

    dev = torch.device("cuda", 0)
    n = a.lanes
    es, ps = list(range(n)), list(range(1_000_000, 1_000_000 + n))
    out = {"device": torch.cuda.get_device_name(0), "lanes": n, "max_steps": a.max_steps, "cases": []}
    for size in (3, 5, 8):
        for mode, hidden in (("log2", [64, 64]), ("onehot", [256, 128, 64])):
            cfg = Game2048EnvConfig(size=size, obs_mode=mode, obs_log2_scale=0.0625, reward_mode="log2",
                                    base_reward_scale=0.5, max_steps=a.max_steps)
            agent = ReinforceAgent(cfg, MLPConfig(hidden_sizes=hidden, activation="ReLU", init_distribution="HeNormal"),
                                   ReinforceAgentConfig(model_seed=1, gamma=0.99, baseline_mode="batch", use_critic=True),
                                   device=dev)
            agent.use_fused_sized_rollout = True
            batch = agent.rollout_batch(es, ps)
            steps = int(batch.lengths.sum())
            keep = [{k: [t.clone() for t in v] for k, v in P.items()} for P in (agent.params, agent.critic_params)]
            fused = "g2048_sized_grad" + (" + g2048_sized_onehot_dw1" if mode == "onehot" else "")

            def update(on: bool):
                agent.params = {k: [t.clone() for t in v] for k, v in keep[0].items()}
                agent.critic_params = {k: [t.clone() for t in v] for k, v in keep[1].items()}
                agent._params_version += 1
                agent.use_fused_sized_grad = on
                torch.cuda.synchronize()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                agent.update_from_batch(batch)
                e.record()
                torch.cuda.synchronize()
                p = agent.last_paths()
                assert p["actor_grad"] == p["critic_grad"] == (fused if on else GENERAL), p
                return s.elapsed_time(e)

            grads = {}
            for on in (False, True):                                      # warm-up 1 + the comparison
                update(on)
                grads[on] = [g.double() for g in agent.last_grads["actor"] + agent.last_grads["critic"]]
            diff = max(float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)) for x, y in zip(grads[True], grads[False]))
            for on in (False, True):                                      # warm-up 2
                update(on)
            ms = {False: [], True: []}
            for _ in range(a.repeats):
                for on in (False, True):
                    ms[on].append(update(on))
            g, f = summary(ms[False]), summary(ms[True])
            spread = (g["p90_ms"] - g["p10_ms"]) + (f["p90_ms"] - f["p10_ms"])
            case = {"size": size, "obs": mode, "hidden": hidden, "board_steps": steps, "general": g, "fused": f,
                    "general_over_fused": g["median_ms"] / f["median_ms"],
                    "beats_general_by_more_than_spread": bool(g["median_ms"] - f["median_ms"] > spread),
                    "max_normwise_gradient_difference": diff}
            out["cases"].append(case)
            print(json.dumps(case), flush=True)
            del agent, batch
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    sys.exit(main())
