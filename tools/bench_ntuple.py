"""TOOL: env steps/s of the n-tuple players (evaluate_batch with action_gen = NTuplePolicy) against the expectimax player
of the same depth in the same process, and rows/s of the TD(0) update (GPU box).

    python tools/bench_ntuple.py [--weights trained.npz] [--calls 5] [--warmup 1] [--out profiles/ntuple/bench_ntuple.json]

One process, one device, the default env (max_steps None: every episode runs to its end).  The protocol of
tools/bench_search.py: per case `--warmup` calls per player, then `--calls` calls per player ALTERNATING the two on one
fixed seed list, one HIP event pair per call; median and min-max over the calls, every call kept in the file.  Depth-1
cases above 4,096 episodes make `--calls-deep` calls and are warmed by the smaller cases before them.  Every call's
lengths and totals must equal the first call's of that player on those seeds (asserted).

Cases: 4 x 4 depth 0 against ExpectimaxPolicy(depth=0) and depth 1 against ExpectimaxPolicy(depth=1) (the per-lane
kernels) at n = 64, 2,048 and 65,536; N = 5 depth 0.  Weights: the closed-form hash (seed 104 at 4 x 4), or with
--weights a state_dict saved by tools/train_ntuple.py (4 x 4 only; learned play makes longer episodes) -- "weights" in
the file says which.

Update: one rollout_batch of 65,536 episodes by the depth-0 player, then ntuple_update on it `--calls` times from the
same weights (restored before every call; the weights after every call must be identical) at the rate
2^-`--update-lr-shift` (a row whose step rounds to 0 issues no atomics, so the rate decides how many adds are
measured), against the same kernel on
a batch of the same shape whose boards are shuffled random fills and whose actions are random: the hot entries of
mostly-empty tuples are gone there, so the ratio shows what same-address contention costs.  Also the update's share of
one rollout + update iteration.
"""
import argparse
import dataclasses
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(calls: list, keys) -> dict:
    out = {"calls": calls}
    for k in keys:
        v = np.array([c[k] for c in calls])
        out[k + "_median"], out[k + "_min"], out[k + "_max"] = float(np.median(v)), float(v.min()), float(v.max())
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return r, e0.elapsed_time(e1) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--calls-deep", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="4:0,4:1,5:0", help="size:depth, comma separated")
    ap.add_argument("--ns", default="64,2048,65536")
    ap.add_argument("--depth1-max-n", type=int, default=65536, help="skip depth-1 cases above this many episodes")
    ap.add_argument("--update-episodes", type=int, default=65536)
    ap.add_argument("--update-lr-shift", type=int, default=10,
                    help="the update's rate is 2^-this: a row whose step rounds to 0 issues no atomics, so a small rate "
                         "measures the kernel without its adds (2^-21 on hash weights: most rows)")
    ap.add_argument("--weights", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntuple", "bench_ntuple.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ntuple needs a HIP device: a timing taken elsewhere says nothing")
    from rl2048_amd import ExpectimaxPolicy, Game2048EnvConfig, NTupleNetwork, NTuplePolicy
    from rl2048_amd.agent import ReinforceAgent, ReinforceAgentConfig
    from rl2048_amd.mlp import MLPConfig

    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "calls": a.calls, "calls_deep": a.calls_deep, "warmup": a.warmup,
           "weights": "hash (seed 100 + N)" if a.weights is None else "trained: " + os.path.basename(a.weights),
           "cases": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    def network(size):
        net = NTupleNetwork(size, device=dev)
        if a.weights is None:
            net.fill_hash(100 + size)
        else:
            with np.load(a.weights) as z:
                net.load_state_dict({k: z[k] for k in z.files})
        return net

    def agent_of(size):
        return ReinforceAgent(Game2048EnvConfig(size=size, max_steps=None), MLPConfig(hidden_sizes=[8], activation="ReLU"),
                              ReinforceAgentConfig(model_seed=0), device=dev)

    for case in [c for c in a.cases.split(",") if c]:
        size, depth = (int(x) for x in case.split(":"))
        if a.weights is not None and size != 4:
            continue
        agent, net = agent_of(size), network(size)
        players = {"ntuple": NTuplePolicy(net, depth), "expectimax": ExpectimaxPolicy(depth=depth)}
        for n in (int(x) for x in a.ns.split(",")):
            if depth >= 1 and n > a.depth1_max_n:
                continue
            es = np.arange(n, dtype=np.int64)
            ps = es + 1_000_000
            score, first = {}, {}

            def one(who: str) -> dict:
                b, t = timed(lambda: agent.evaluate_batch(es, ps, action_gen=players[who]))
                if who not in first:
                    first[who] = (b.lengths.clone(), b.total_reward.clone())
                assert torch.equal(b.lengths, first[who][0]) and torch.equal(b.total_reward, first[who][1]), \
                    f"{who}: two calls on the same seeds differ"
                steps = int(b.lengths.sum().item())
                mt = b.max_tile.cpu().numpy()
                score[who] = {"steps": steps, "mean_total_reward": float(b.total_reward.mean().item()),
                              "mean_length": steps / n, "share_2048": float((mt >= 2048).mean())}
                return {"time_s": t, "steps_per_s": steps / t, "episodes_per_s": n / t}

            deep = depth >= 1 and n > 4096
            calls = {who: [] for who in players}
            for _ in range(0 if deep else a.warmup):
                for who in players:
                    one(who)
            for _ in range(a.calls_deep if deep else a.calls):
                for who in players:                 # alternating: both players see the same box
                    calls[who].append(one(who))
            keys = ("steps_per_s", "episodes_per_s", "time_s")
            res = {who: dict(stats(c, keys), **score[who]) for who, c in calls.items()}
            res["warmup"] = "the smaller cases of the same players" if deep else f"{a.warmup} call(s) of this case"
            res["path_of_ntuple_call"] = agent._PERSISTENT["sized_ntuple" if size != 4 else "ntuple"].eval_path
            res["steps_per_s_ntuple_over_expectimax"] = \
                res["ntuple"]["steps_per_s_median"] / res["expectimax"]["steps_per_s_median"]
            out["cases"][f"N{size}-depth{depth}-n{n}"] = res
            print(f"N{size} depth {depth} n {n}: " + ", ".join(
                f"{w} {res[w]['steps_per_s_median'] / 1e6:.3f} M steps/s ({res[w]['steps_per_s_min'] / 1e6:.3f}-"
                f"{res[w]['steps_per_s_max'] / 1e6:.3f}), {res[w]['time_s_median']:.3f} s, mean score "
                f"{res[w]['mean_total_reward']:.0f}, mean length {res[w]['mean_length']:.0f}" for w in players), flush=True)
            save()

    # ------------------------------------------------------------------------------------------------ the update
    n = a.update_episodes
    agent, net = agent_of(4), network(4)
    pol = NTuplePolicy(net, 0)
    es = np.arange(n, dtype=np.int64) + 5_000_000
    for _ in range(a.warmup):
        agent.rollout_batch(es[:4096], es[:4096] + 1, action_gen=pol)
    batch, t_roll = timed(lambda: agent.rollout_batch(es, es + 1, action_gen=pol))
    rows_valid = int(batch.lengths.sum().item())
    # the same shape, without the structure: every valid row a shuffled random fill, a random action
    g = torch.Generator(device=dev).manual_seed(1)
    T = batch.T
    fill = torch.rand(T, n, device=dev, generator=g) * 0.7 + 0.3
    boards = torch.zeros(T, n, dtype=torch.int64, device=dev)
    for cell in range(16):
        e = torch.randint(1, 12, (T, n), device=dev, generator=g) * (torch.rand(T, n, device=dev, generator=g) < fill)
        boards |= e << (4 * cell)
    rand = dataclasses.replace(batch, boards=boards,
                               actions=torch.randint(0, 4, (T, n), device=dev, generator=g).to(torch.uint8))
    del e, fill, boards
    before = net.weights.clone()
    res = {}
    for name, b in (("played", batch), ("random_fills", rand)):
        calls, after = [], None
        for k in range(a.warmup + a.calls):
            net.weights.copy_(before)
            st, t = timed(lambda: agent.ntuple_update(b, net, 1, a.update_lr_shift))
            if after is None:
                after = net.weights.clone()
            assert torch.equal(net.weights, after), f"{name}: two updates from the same weights differ"
            if k >= a.warmup:
                calls.append({"time_s": t, "rows_per_s": st["rows"] / t})
        res[name] = dict(stats(calls, ("rows_per_s", "time_s")), rows=st["rows"], abs_delta=st["abs_delta"],
                         weights_changed=int((after != before).sum().item()))
    net.weights.copy_(before)
    res.update(episodes=n, T=T, rows_valid=rows_valid, lr_num=1, lr_shift=a.update_lr_shift, rollout_time_s=t_roll, path=agent.last_paths()["ntuple_update"],
               update_share_of_iteration=res["played"]["time_s_median"] / (res["played"]["time_s_median"] + t_roll),
               rows_per_s_played_over_random=res["played"]["rows_per_s_median"] / res["random_fills"]["rows_per_s_median"])
    out["update"] = res
    print(f"update on {n} episodes (T {T}, {rows_valid} rows): played {res['played']['rows_per_s_median'] / 1e6:.1f} M "
          f"rows/s ({res['played']['time_s_median'] * 1e3:.1f} ms), random fills "
          f"{res['random_fills']['rows_per_s_median'] / 1e6:.1f} M rows/s; rollout {t_roll:.3f} s, update share "
          f"{100 * res['update_share_of_iteration']:.1f} %", flush=True)
    save()


if __name__ == "__main__":
    main()
