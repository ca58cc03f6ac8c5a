"""TOOL: train an n-tuple value network by afterstate TD(0) on the device and record its learning curve (GPU box).

    python tools/train_ntuple.py [--size 4] [--episodes 4096] [--iterations 100 | --seconds 600] [--lr-num 1]
                                 [--lr-shift 12] [--eval-every 10] [--out profiles/ntuple/train_ntuple.json]
                                 [--save weights.npz]

The loop: rollout_batch(action_gen=NTuplePolicy(net)) on fresh seeds -> ntuple_update(batch, net, lr_num, lr_shift);
every --eval-every iterations (and before the first) evaluate_batch on --eval-episodes FIXED seeds: mean score (total
reward under the default env, the game's score), mean length, the share of episodes whose largest tile reached 2048 and
the max-tile histogram.  Weights start at zero (the greedy-merge player).  Stops after --iterations, or after --seconds
of wall time, whichever comes first.  At the end the final weights are evaluated once more by the depth-1 player on the
first --final-episodes evaluation seeds, beside the greedy player on the same seeds.

Choosing the rate (DESIGN.md section 3 has the runs).  One update adds the steps of EVERY row of the batch to weights
read before the call, so an entry hit by M rows moves by lr * the sum of M deltas, and the entries of the first moves'
boards are hit by every episode: the larger the batch, the smaller the rate that does not overshoot.  Against that, a
step is an integer in units of 2^-10 points: a row registers only if |delta| * lr >= 1 unit, and negative deltas floor
to -1.  At 4,096 episodes the bound first derived from the overshoot, 2^-21, moved no weight at all in 11,379
iterations, and 2^-18, 2^-15 and 2^-12 (the default here: the least bad of the runs, not a recommendation) all ended
below the zero-weight player.  Nothing in this tool tunes anything.
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


def summary(b, n: int) -> dict:
    mt = b.max_tile.cpu().numpy()
    return {"mean_score": float(b.total_reward.mean().item()), "mean_length": float(b.lengths.sum().item()) / n,
            "share_2048": float((mt >= 2048).mean()),
            "max_tile_counts": {int(t): int((mt == t).sum()) for t in sorted(set(mt.tolist()))}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4)
    ap.add_argument("--episodes", type=int, default=4096)
    ap.add_argument("--eval-episodes", type=int, default=4096)
    ap.add_argument("--final-episodes", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--eval-every", type=int, default=10)
    ap.add_argument("--lr-num", type=int, default=1)
    ap.add_argument("--lr-shift", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntuple", "train_ntuple.json"))
    ap.add_argument("--save", default=None, help="write the final state_dict here (.npz)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("train_ntuple needs a HIP device")
    from rl2048_amd import Game2048EnvConfig, NTupleNetwork, NTuplePolicy
    from rl2048_amd.agent import ReinforceAgent, ReinforceAgentConfig
    from rl2048_amd.mlp import MLPConfig

    dev = torch.device("cuda", 0)
    agent = ReinforceAgent(Game2048EnvConfig(size=a.size, max_steps=None), MLPConfig(hidden_sizes=[8], activation="ReLU"),
                           ReinforceAgentConfig(model_seed=0), device=dev)
    net = NTupleNetwork(a.size, device=dev)
    greedy, deeper = NTuplePolicy(net, 0), NTuplePolicy(net, 1)
    ev_e = np.arange(a.eval_episodes, dtype=np.int64) + 10 ** 12
    out = {"device": torch.cuda.get_device_name(0), "size": a.size, "episodes": a.episodes,
           "eval_episodes": a.eval_episodes, "lr_num": a.lr_num, "lr_shift": a.lr_shift, "features": len(net.features),
           "weights": net.n_weights, "recorded_expectimax_means": {"depth1": 16320, "depth2": 24697}, "curve": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    def evaluate(it: int, rows: int, t_train: float) -> None:
        s = summary(agent.evaluate_batch(ev_e, ev_e + 1, action_gen=greedy), a.eval_episodes)
        s.update(iteration=it, rows_trained=rows, train_seconds=t_train)
        out["curve"].append(s)
        print(f"iteration {it}: mean score {s['mean_score']:.0f}, mean length {s['mean_length']:.0f}, reached 2048 "
              f"{100 * s['share_2048']:.2f} %, {rows} rows in {t_train:.1f} s", flush=True)
        save()

    t0, rows, t_train, it = time.time(), 0, 0.0, 0
    evaluate(0, 0, 0.0)
    while it < a.iterations and time.time() - t0 < a.seconds:
        es = np.arange(a.episodes, dtype=np.int64) + (it + 1) * 10 ** 7
        torch.cuda.synchronize()
        t1 = time.time()
        batch = agent.rollout_batch(es, es + 1, action_gen=greedy)
        st = agent.ntuple_update(batch, net, a.lr_num, a.lr_shift)      # reads the stats back: synchronises
        t_train += time.time() - t1
        rows += st["rows"]
        del batch
        it += 1
        if it % a.eval_every == 0:
            evaluate(it, rows, t_train)
    if it % a.eval_every:
        evaluate(it, rows, t_train)
    out["iterations"] = it
    out["paths"] = agent.last_paths()
    k = min(a.final_episodes, a.eval_episodes)
    out["final"] = {"episodes": k,
                    "greedy": summary(agent.evaluate_batch(ev_e[:k], ev_e[:k] + 1, action_gen=greedy), k),
                    "depth1": summary(agent.evaluate_batch(ev_e[:k], ev_e[:k] + 1, action_gen=deeper), k)}
    print(f"final weights on {k} seeds: greedy {out['final']['greedy']['mean_score']:.0f}, depth 1 "
          f"{out['final']['depth1']['mean_score']:.0f}", flush=True)
    save()
    if a.save:
        os.makedirs(os.path.dirname(os.path.abspath(a.save)), exist_ok=True)
        np.savez_compressed(a.save, **net.state_dict())


if __name__ == "__main__":
    main()
