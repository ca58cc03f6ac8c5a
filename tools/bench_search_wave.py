"""TOOL: the expectimax player one episode per lane (g2048_*search_eval) against one episode per wave
(g2048_*search_wave_eval; ReinforceAgent.search_cooperative) on the same seeds in one process (GPU box).

    python tools/bench_search_wave.py [--calls 3] [--warmup 1] [--out profiles/search/bench_search_wave.json]

tools/bench_search.py's protocol: one process, one device, the default env (max_steps None: every episode runs to its
end), evaluate_batch, one HIP event pair per call.  Cases (`--cases size:depth:n,...`): 4 x 4 depth 1 at n = 64, 2,048,
65,536 and 524,288 (past the crossover), 4 x 4 depth 2 at n = 1, 64 and 2,048, N = 5 depth 1 at n = 64 and 2,048; the
per-lane depth-2 calls last 6 to 51 s each, the whole list about nine minutes.  Per case `--warmup` calls per
side, then `--calls` timed calls per side ALTERNATING the two; calls/s, episodes/s and env steps/s are reported as
median and min-max, and the file keeps every call with the longest single launch it saw (one event pair per launch of
the driver).  The two sides must give the same lengths, totals (by bits), max tiles and final boards: the tool asserts
it, so every timing is also an end-to-end check.  `won` is true where the cooperative side's slowest call beats the
per-lane side's fastest (the medians differ by more than both spreads together).  Nothing is tuned per case.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_CASES = "4:1:64,4:1:2048,4:1:65536,4:1:524288,4:2:1,4:2:64,4:2:2048,5:1:64,5:1:2048"
SIDES = ("per_lane", "cooperative")


def stats(calls: list) -> dict:
    out = {"calls": calls}
    for k in ("time_s", "calls_per_s", "episodes_per_s", "steps_per_s", "longest_launch_s"):
        v = np.array([c[k] for c in calls])
        out[k + "_median"], out[k + "_min"], out[k + "_max"] = float(np.median(v)), float(v.min()), float(v.max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default=DEFAULT_CASES, help="size:depth:n, comma separated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search", "bench_search_wave.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_search_wave needs a HIP device: a timing taken elsewhere says nothing")
    from rl2048_amd import ExpectimaxPolicy, Game2048EnvConfig, rollouts
    from rl2048_amd.agent import ReinforceAgent, ReinforceAgentConfig
    from rl2048_amd.mlp import MLPConfig

    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "calls": a.calls, "warmup": a.warmup,
           "search_step_budget": ReinforceAgent.search_step_budget, "cases": {}}
    if os.path.exists(a.out):               # a run of some cases adds to the file
        with open(a.out) as f:
            out["cases"] = json.load(f).get("cases", {})

    # one event pair per launch of the score-only driver: the longest launch of a call
    launches = []
    run_budgeted = rollouts.run_budgeted

    def timed_run_budgeted(launch, *rest):
        def timed(*args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch(*args)
            e1.record()
            launches.append((e0, e1))
        return run_budgeted(timed, *rest)

    rollouts.run_budgeted = timed_run_budgeted
    agents = {}
    for case in a.cases.split(","):
        size, depth, n = (int(x) for x in case.split(":"))
        if size not in agents:
            agents[size] = ReinforceAgent(Game2048EnvConfig(size=size, max_steps=None),
                                          MLPConfig(hidden_sizes=[8], activation="ReLU"),
                                          ReinforceAgentConfig(model_seed=0), device=dev)
        agent, pol = agents[size], ExpectimaxPolicy(depth=depth)
        es = np.arange(n, dtype=np.int64)
        ps = es + 1_000_000
        result, paths = {}, {}

        def one(side: str) -> dict:
            agent.search_cooperative = side == "cooperative"
            launches.clear()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            b = agent.evaluate_batch(es, ps, action_gen=pol)
            e1.record()
            torch.cuda.synchronize()
            t = e0.elapsed_time(e1) * 1e-3
            result[side], paths[side] = b, agent.last_paths()["eval"]
            steps = int(b.lengths.sum().item())
            return {"time_s": t, "calls_per_s": 1.0 / t, "episodes_per_s": n / t, "steps": steps,
                    "steps_per_s": steps / t, "launches": len(launches),
                    "longest_launch_s": max(x.elapsed_time(y) for x, y in launches) * 1e-3}

        for _ in range(a.warmup):
            for side in SIDES:
                one(side)
        calls = {side: [] for side in SIDES}
        for _ in range(a.calls):
            for side in SIDES:                  # alternating: both sides see the same box
                calls[side].append(one(side))
        x, y = result["per_lane"], result["cooperative"]
        assert "per lane" in paths["per_lane"] and "per wave" in paths["cooperative"], paths
        assert torch.equal(x.lengths, y.lengths) and torch.equal(x.max_tile, y.max_tile)
        assert torch.equal(x.total_reward.view(torch.int64), y.total_reward.view(torch.int64))
        assert torch.equal(x.final_boards, y.final_boards)
        res = {side: stats(c) for side, c in calls.items()}
        mt = y.max_tile.cpu().numpy()
        res.update(steps=int(y.lengths.sum().item()), mean_length=float(y.lengths.double().mean().item()),
                   mean_total_reward=float(y.total_reward.mean().item()),
                   max_tile_counts={int(t): int((mt == t).sum()) for t in sorted(set(mt.tolist()))},
                   results_identical=True, paths=paths,
                   speedup_median=res["per_lane"]["time_s_median"] / res["cooperative"]["time_s_median"],
                   won=res["cooperative"]["time_s_max"] < res["per_lane"]["time_s_min"],
                   lost=res["cooperative"]["time_s_min"] > res["per_lane"]["time_s_max"])
        out["cases"][f"N{size}-depth{depth}-n{n}"] = res
        print(f"N{size} depth {depth} n {n}: " + ", ".join(
            f"{s} {res[s]['time_s_median']:.4f} s ({res[s]['time_s_min']:.4f}-{res[s]['time_s_max']:.4f}), "
            f"{res[s]['calls_per_s_median']:.3f} calls/s, {res[s]['steps_per_s_median']:.0f} steps/s, longest launch "
            f"{res[s]['longest_launch_s_max']:.3f} s" for s in SIDES) +
            f"; x{res['speedup_median']:.2f}, won {res['won']}, lost {res['lost']}, results identical", flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
