"""TOOL: the fused sized gradient (use_fused_sized_grad) against fp64 at tools/bench_sized_grad.py's sample count (GPU box).

    python tools/check_sized_grad_at_size.py [--lanes 65536] [--max-steps 64] > profiles/sized/sized_grad_at_size.txt

Per case one rollout of `--lanes` episodes and one update on each path from the same parameters; the fp64 value is
tests/sized_grad_ref.py's _exact_update under the fused kernel's own ReLU pattern, with the pattern's flips against
fp64's own counted and bounded (EG.pattern_flip_check_deep).  Prints, per case, the largest normwise error of the fused
path, the general path's distance from the same value, and the flip counts per layer.
Cases: N = 5 and 8 log2 [64, 64], N = 3 one-hot [256, 128, 64], ReLU, actor-critic (MSE).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = ((5, "log2", [64, 64]), (8, "log2", [64, 64]), (3, "onehot", [256, 128, 64]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--max-steps", type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("check_sized_grad_at_size needs a HIP device")
    import exact_grad as EG
    from sized_grad_ref import _exact_update

    from rl2048_amd import Game2048EnvConfig
    from rl2048_amd.agent import ReinforceAgent, ReinforceAgentConfig
    from rl2048_amd.mlp import MLPConfig

    dev = torch.device("cuda", 0)
    n = a.lanes
    es, ps = list(range(n)), list(range(1_000_000, 1_000_000 + n))
    for size, mode, hidden in CASES:
        cfg = Game2048EnvConfig(size=size, obs_mode=mode, obs_log2_scale=0.0625, reward_mode="log2",
                                base_reward_scale=0.5, max_steps=a.max_steps)
        grads, flips, exact = {}, {}, None
        for on in (True, False):
            agent = ReinforceAgent(cfg, MLPConfig(hidden_sizes=hidden, activation="ReLU", init_distribution="HeNormal"),
                                   ReinforceAgentConfig(model_seed=1, gamma=0.99, baseline_mode="batch", use_critic=True),
                                   device=dev)
            agent.use_fused_sized_rollout = True
            batch = agent.rollout_batch(es, ps)
            snap = EG.snapshot(agent)
            agent.use_fused_sized_grad = on
            agent.update_from_batch(batch)
            grads[on] = agent.last_grads
            if on:
                exact = _exact_update(agent, batch, snap, flips)
            del agent, batch
        print(json.dumps({"size": size, "obs": mode, "hidden": hidden,
                          "fused_vs_fp64_kernel_pattern": max(EG.grad_errors(grads[True], exact).values()),
                          "general_vs_fp64_fused_pattern": max(EG.grad_errors(grads[False], exact).values()),
                          "flips": {k: {"n": v["n"], "tot": v["tot"], "viol": v["viol"]} for k, v in flips.items()}}),
              flush=True)
        del exact
        torch.cuda.empty_cache()


if __name__ == "__main__":
    sys.exit(main())
