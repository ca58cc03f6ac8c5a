"""TOOL: env steps/s of scripted play (rollout_batch / evaluate_batch with action_gen) against the fastest net-driven
way to play the same number of episodes (GPU box).

    python tools/bench_scripted.py [--episodes 65536] [--calls 10] [--warmup 2] [--out profiles/scripted/bench_scripted.json]

One process, one device, the default env (max_steps None; obs log2 so that the net-driven path applies), 4 x 4 and
N = 5, `--episodes` episodes on one fixed seed list.  Per size and form (evaluate_batch = score-only, rollout_batch =
trajectory) three paths:
  urld      action_gen = PriorityPolicy(URLD)           g2048_scripted_* / g2048_sized_scripted_*
  uniform   action_gen = UniformPolicy()                the same kernels
  net8      a log2 [8] ReLU net, greedy                 g2048_deep_* (4 x 4) / g2048_sized_* with use_fused_sized_rollout
`--warmup` calls per path, then `--calls` calls per path ALTERNATING the paths, one HIP event pair per call.  The
episodes differ in length between the paths (a scripted player lasts longer than an untrained net), so the figure is
env steps/s = sum(lengths) / time, reported as median and p10-p90 over the calls; the file keeps every call.  Also the
host run_episode(action_gen=<plain callable>) loop on 32 episodes, in episodes/s, for scale.  Nothing is tuned per
path; no share of peak is claimed (the kernel is latency-bound integer / fp64 VALU work: see DESIGN.md).
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


def stats(calls: list) -> dict:
    r = np.array([c["steps_per_s"] for c in calls])
    return {"steps_per_s_median": float(np.median(r)), "steps_per_s_p10": float(np.percentile(r, 10)),
            "steps_per_s_p90": float(np.percentile(r, 90)), "time_s_median": float(np.median([c["time_s"] for c in calls])),
            "steps": int(calls[0]["steps"]), "calls": calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="4,5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scripted", "bench_scripted.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_scripted needs a HIP device: a timing taken elsewhere says nothing")
    from rl2048_amd import Game2048EnvConfig, PriorityPolicy, UniformPolicy
    from rl2048_amd.agent import ReinforceAgent, ReinforceAgentConfig
    from rl2048_amd.mlp import MLPConfig

    dev = torch.device("cuda", 0)
    n = a.episodes
    es = np.arange(n, dtype=np.int64)
    ps = es + 1_000_000
    players = {"urld": PriorityPolicy(PriorityPolicy.URLD), "uniform": UniformPolicy(), "net8": None}
    out = {"device": torch.cuda.get_device_name(0), "episodes": n, "calls": a.calls, "warmup": a.warmup, "cases": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    for size in (int(s) for s in a.sizes.split(",")):
        cfg = Game2048EnvConfig(size=size, obs_mode="log2", max_steps=None)
        agent = ReinforceAgent(cfg, MLPConfig(hidden_sizes=[8], activation="ReLU", init_distribution="HeNormal"),
                               ReinforceAgentConfig(model_seed=0), device=dev)
        agent.use_fused_sized_rollout = True

        def one(form: str, who: str) -> dict:
            play = agent.evaluate_batch if form == "evaluate_batch" else agent.rollout_batch
            kw = dict(use_greedy=True) if players[who] is None else dict(action_gen=players[who])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            b = play(es, ps, **kw)
            e1.record()
            torch.cuda.synchronize()
            t = e0.elapsed_time(e1) * 1e-3
            steps = int(b.lengths.sum().item())
            del b
            return {"time_s": t, "steps": steps, "steps_per_s": steps / t}

        for form in ("evaluate_batch", "rollout_batch"):
            calls = {who: [] for who in players}
            for _ in range(a.warmup):
                for who in players:
                    one(form, who)
            paths = dict(agent.last_paths())
            for _ in range(a.calls):
                for who in players:                 # alternating: every path sees the same box
                    calls[who].append(one(form, who))
            case = {who: stats(c) for who, c in calls.items()}
            case["path_of_last_call"] = paths["eval" if form == "evaluate_batch" else "rollout"]
            net = case["net8"]
            for who in ("urld", "uniform"):
                s = case[who]
                spreads = (s["steps_per_s_p90"] - s["steps_per_s_p10"]) + (net["steps_per_s_p90"] - net["steps_per_s_p10"])
                s["over_net8"] = s["steps_per_s_median"] / net["steps_per_s_median"]
                s["exceeds_net8_by_more_than_both_spreads"] = bool(
                    s["steps_per_s_median"] - net["steps_per_s_median"] > spreads)
            out["cases"][f"N{size}-{form}"] = case
            print(f"N{size} {form}: " + ", ".join(
                f"{w} {case[w]['steps_per_s_median'] / 1e6:.1f} M steps/s ({case[w]['steps_per_s_p10'] / 1e6:.1f}-"
                f"{case[w]['steps_per_s_p90'] / 1e6:.1f}), {case[w]['time_s_median']:.3f} s" for w in players), flush=True)
            save()
        # the host loop (run_episode with a plain callable), for scale
        t0 = time.perf_counter()
        steps = 0
        for i in range(32):
            tr = agent.run_episode(int(es[i]), int(ps[i]), action_gen=lambda s, m: next(k for k in (0, 1, 3, 2) if m[k]))
            steps += len(tr["actions"])
        dt = time.perf_counter() - t0
        out["cases"][f"N{size}-host_run_episode"] = {"episodes": 32, "steps": steps, "wall_s": dt,
                                                     "episodes_per_s": 32 / dt, "steps_per_s": steps / dt}
        print(f"N{size} host run_episode loop: {32 / dt:.2f} episodes/s, {steps / dt:.0f} steps/s", flush=True)
        save()


if __name__ == "__main__":
    main()
