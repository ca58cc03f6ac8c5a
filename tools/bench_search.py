"""TOOL: env steps/s and episodes/s of the expectimax player (evaluate_batch with action_gen = ExpectimaxPolicy)
against PriorityPolicy.URLD in the same process, and what each player scores on the same seeds (GPU box).

    python tools/bench_search.py [--calls 5] [--warmup 1] [--out profiles/search/bench_search.json]

One process, one device, the default env (max_steps None: every episode runs to its end).  Cases: depth 0, 1, 2 at
4 x 4 and depth 1 at N = 5, each at n = 64, 2,048 and 65,536 episodes on one fixed seed list (`--cases` / `--ns` select
fewer).  Per case `--warmup` calls per player, then `--calls` calls per player ALTERNATING the two, one HIP event pair
per call.  A depth-2 call at 65,536 episodes takes minutes: `--calls-deep` calls there, and its warm-up is the smaller
cases of the same player run before it in this process (the kernel is loaded and has run); when there is none, one
64-episode call of the player is made first.  Every case records which it was ("warmup").  The players' episodes
differ in length (a lookahead player lasts longer), so both env steps/s = sum(lengths) / time and episodes/s are
reported, as median and min-max over the calls; the file keeps every call.  The mean total reward (the game score
under the default reward) and the max-tile histogram come from the same calls' results.  Nothing is tuned per case; no
share of peak is claimed (integer VALU work, one episode per lane: see DESIGN.md).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(calls: list) -> dict:
    out = {"steps": int(calls[0]["steps"]), "calls": calls}
    for k in ("steps_per_s", "episodes_per_s", "time_s"):
        v = np.array([c[k] for c in calls])
        out[k + "_median"], out[k + "_min"], out[k + "_max"] = float(np.median(v)), float(v.min()), float(v.max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--calls-deep", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="4:0,4:1,4:2,5:1", help="size:depth, comma separated")
    ap.add_argument("--ns", default="64,2048,65536")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search", "bench_search.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_search needs a HIP device: a timing taken elsewhere says nothing")
    from rl2048_amd import ExpectimaxPolicy, Game2048EnvConfig, PriorityPolicy
    from rl2048_amd.agent import ReinforceAgent, ReinforceAgentConfig
    from rl2048_amd.mlp import MLPConfig

    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "calls": a.calls, "calls_deep": a.calls_deep, "warmup": a.warmup,
           "cases": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    for case in a.cases.split(","):
        size, depth = (int(x) for x in case.split(":"))
        agent = ReinforceAgent(Game2048EnvConfig(size=size, max_steps=None), MLPConfig(hidden_sizes=[8], activation="ReLU"),
                               ReinforceAgentConfig(model_seed=0), device=dev)
        players = {"search": ExpectimaxPolicy(depth=depth), "urld": PriorityPolicy(PriorityPolicy.URLD)}
        warmed = False
        for n in (int(x) for x in a.ns.split(",")):
            es = np.arange(n, dtype=np.int64)
            ps = es + 1_000_000
            score = {}

            def one(who: str) -> dict:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                b = agent.evaluate_batch(es, ps, action_gen=players[who])
                e1.record()
                torch.cuda.synchronize()
                t = e0.elapsed_time(e1) * 1e-3
                steps = int(b.lengths.sum().item())
                mt = b.max_tile.cpu().numpy()
                score[who] = {"mean_total_reward": float(b.total_reward.mean().item()),
                              "mean_length": steps / n,
                              "max_tile_counts": {int(t_): int((mt == t_).sum()) for t_ in sorted(set(mt.tolist()))}}
                return {"time_s": t, "steps": steps, "steps_per_s": steps / t, "episodes_per_s": n / t}

            deep = depth == 2 and n > 4096
            calls = {who: [] for who in players}
            if deep and not warmed:
                agent.evaluate_batch(es[:64], ps[:64], action_gen=players["search"])
                agent.evaluate_batch(es[:64], ps[:64], action_gen=players["urld"])
            warm = ("earlier cases of the same player in this process" if warmed else "one 64-episode call") if deep \
                else f"{a.warmup} call(s) of this case"
            for _ in range(0 if deep else a.warmup):
                for who in players:
                    one(who)
            warmed = True
            for _ in range(a.calls_deep if deep else a.calls):
                for who in players:                 # alternating: both players see the same box
                    calls[who].append(one(who))
                    if calls[who][-1]["time_s"] > 5.0:
                        print(f"  N{size} depth {depth} n {n} {who}: {calls[who][-1]['time_s']:.1f} s", flush=True)
            res = {who: dict(stats(c), **score[who]) for who, c in calls.items()}
            res["warmup"] = warm
            res["path_of_search_call"] = agent._PERSISTENT["sized_search" if size != 4 else "search"].eval_path
            res["steps_per_s_search_over_urld"] = res["search"]["steps_per_s_median"] / res["urld"]["steps_per_s_median"]
            out["cases"][f"N{size}-depth{depth}-n{n}"] = res
            print(f"N{size} depth {depth} n {n}: " + ", ".join(
                f"{w} {res[w]['steps_per_s_median'] / 1e6:.3f} M steps/s ({res[w]['steps_per_s_min'] / 1e6:.3f}-"
                f"{res[w]['steps_per_s_max'] / 1e6:.3f}), {res[w]['episodes_per_s_median']:.0f} episodes/s, "
                f"{res[w]['time_s_median']:.3f} s, mean score {res[w]['mean_total_reward']:.0f}, tiles "
                f"{res[w]['max_tile_counts']}" for w in players), flush=True)
            save()


if __name__ == "__main__":
    main()
