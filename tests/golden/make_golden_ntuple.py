"""Generate the n-tuple value network fixtures from the REAL reference (build container only).

    python tests/golden/make_golden_ntuple.py [--ref /root/reference]

Imports the reference the way make_golden_ref.py does and writes tests/golden/ntuple.npz (data only; no weights are
stored, only the seeds of the closed-form hash that rebuilds them).  The model is written out here on its own (below:
include/g2048_ntuple.h's definition in plain Python and numpy, no project code), its move is first checked against the
reference's Game2048._move, and the reference plays it:

  episodes    e{c}_*: ReinforceAgent.run_episode(env_seed, policy_seed, action_gen=Player(...)), 2 episodes per case,
              in search.npz's per-case format.  Cases ("ep_cases", JSON, each with its depth): 4 x 4 depth 0 default
              config; 4 x 4 depth 1 on R-raw-mask with max_steps 60; N = 2 and 3 depth 0; N = 5 depth 0 with max_steps
              40; N = 8 depth 0 with max_steps 48; N = 3 depth 1 with the mask off.  Every episode is run a second time
              under another policy seed and must not differ.
  boards      b{N}_boards [m, N*N] uint8 exponents for N in 2, 3, 4, 5, 8: make_golden_search.py's classes (random
              fills, full, dead, one valid move, transpose-symmetric ties), b{N}_v [m] int64 (V of the board),
              b{N}_q0 [m, 4] int64 (INT64_MIN for an invalid action), b{N}_a0 [m] uint8, and on the subset b{N}_i1
              (every board for N <= 4, where Python is quick enough) b{N}_q1 / b{N}_a1.
  TD          td{N}_* for N in 3, 4: 6 recorded episodes (boards, actions, lengths, whether each ended terminated),
              the learning rate, and what one update gives: td{N}_rows, td{N}_abs_delta and the weight differences,
              sparse, as td{N}_pos / td{N}_val -- computed with np.add.at from the statement in the header.
  weights     hash_seed[N] = HASH_SEED + N for every N.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_ref as MR  # noqa: E402
from make_golden import seed_iter  # noqa: E402
from make_golden_scripted import R_RAW_MASK, TERMS, exponents  # noqa: E402
from make_golden_search import N_RANDOM, special_boards  # noqa: E402

R_LOG2_NOMASK = dict(TERMS, reward_mode="sum", bonus_mode="log2", use_action_mask=False)
F = 10
HASH_SEED = 100
INVALID = -(1 << 63)
BOARD_SIZES = (2, 3, 4, 5, 8)
Q1_STEP = {2: 1, 3: 1, 4: 1, 5: 5, 8: 10}
EPISODES = 2
TD_LR = (3, 5)            # lr_num, lr_shift

EP_CASES = [
    dict(name="4x4-d0-default", size=4, depth=0, env=dict(max_steps=None)),
    dict(name="4x4-d1-terms-60", size=4, depth=1, env=dict(R_RAW_MASK, max_steps=60)),
    dict(name="2x2-d0-terms", size=2, depth=0, env=dict(R_RAW_MASK, max_steps=None)),
    dict(name="3x3-d0-terms", size=3, depth=0, env=dict(R_RAW_MASK, max_steps=None)),
    dict(name="5x5-d0-terms-40", size=5, depth=0, env=dict(R_RAW_MASK, max_steps=40)),
    dict(name="8x8-d0-terms-48", size=8, depth=0, env=dict(R_RAW_MASK, max_steps=48)),
    dict(name="3x3-d1-nomask", size=3, depth=1, env=dict(R_LOG2_NOMASK, max_steps=None)),
]
TD_CASES = {3: dict(max_steps=None), 4: dict(max_steps=48)}


# ------------------------------------------------------------------------------------------------------- the model
def default_tuples(N):
    h, k = (N + 1) // 2, min(N, 4)
    rows = [tuple(r * N + j for j in range(k)) for r in range(h)]
    squares = [(r * N + c, r * N + c + 1, (r + 1) * N + c, (r + 1) * N + c + 1) for r in range(h) for c in range(r, h)]
    return rows + squares


def images(cells, N):
    base = [lambda r, c: (r, c), lambda r, c: (c, N - 1 - r), lambda r, c: (N - 1 - r, N - 1 - c),
            lambda r, c: (N - 1 - c, r)]
    out = []
    for f in base:
        out.append(tuple(f(x // N, x % N)[0] * N + f(x // N, x % N)[1] for x in cells))
    for f in base:
        out.append(tuple(f(x // N, x % N)[1] * N + f(x // N, x % N)[0] for x in cells))
    return out


def hash_table(table, count, seed):
    M = (1 << 64) - 1
    out = np.empty(count, dtype=np.int32)
    for i in range(count):
        x = (seed * 0x9E3779B97F4A7C15 + table * 0xBF58476D1CE4E5B9 + i * 0x94D049BB133111EB + 1) & M
        x ^= x >> 31
        x = (x * 0xD6E8FEB86659FD93) & M
        x ^= x >> 29
        out[i] = (x >> 48) - 32768
    return out


class Net:
    def __init__(self, N, seed):
        self.N = N
        tuples = default_tuples(N)
        offs, off = [], 0
        for t in tuples:
            offs.append(off)
            off += 16 ** len(t)
        self.w = np.concatenate([hash_table(i, 16 ** len(t), seed) for i, t in enumerate(tuples)])
        self.features = [(offs[i], img) for i, t in enumerate(tuples) for img in images(t, N)]
        self.wl = self.w.tolist()

    def positions(self, m):
        return [off + sum(m[c] << (4 * j) for j, c in enumerate(cells)) for off, cells in self.features]

    def V(self, m):
        wl = self.wl
        return sum(wl[p] for p in self.positions(m))


def line_left(cells):
    out, score, i, c = [], 0, 0, [x for x in cells if x]
    while i < len(c):
        if i + 1 < len(c) and c[i] == c[i + 1]:
            assert c[i] < 15, "a 2^15 + 2^15 merge is outside the pinned domain (the device saturates it)"
            out.append(c[i] + 1)
            score += 1 << (c[i] + 1)
            i += 2
        else:
            out.append(c[i])
            i += 1
    return out + [0] * (len(cells) - len(out)), score


def move(b, N, a):
    """b: tuple of N*N exponents, row-major; 0 up, 1 right, 2 down, 3 left -> (board, score gain)."""
    nb, score = list(b), 0
    for k in range(N):
        idx = [k * N + j for j in range(N)] if a in (3, 1) else [j * N + k for j in range(N)]
        if a in (1, 2):
            idx = idx[::-1]
        new, g = line_left([b[i] for i in idx])
        score += g
        for i, v in zip(idx, new):
            nb[i] = v
    return tuple(nb), score


def Q0(net, b):
    qs = []
    for a in range(4):
        m, g = move(b, net.N, a)
        qs.append(INVALID if m == b else (g << F) + net.V(m))
    return qs


def Vmax(net, s):
    return max([q for q in Q0(net, s) if q != INVALID], default=0)


def Q1(net, b):
    qs = []
    for a in range(4):
        m, g = move(b, net.N, a)
        if m == b:
            qs.append(INVALID)
            continue
        tot = E = 0
        for c in range(net.N * net.N):
            if m[c] == 0:
                E += 1
                for k, p in ((1, 9), (2, 1)):
                    nb = list(m)
                    nb[c] = k
                    tot += p * Vmax(net, tuple(nb))
        qs.append((g << F) + tot // (10 * E))
    return qs


def choice(qs):
    best = None
    for a in range(4):
        if qs[a] != INVALID and (best is None or qs[a] > qs[best]):
            best = a
    return 0 if best is None else best


class Player:
    """action_gen for the reference's run_episode: (state, action_mask) -> action."""

    def __init__(self, net, depth):
        self.net, self.depth = net, depth

    def __call__(self, state, action_mask):
        b = tuple(int(v).bit_length() - 1 if v else 0 for row in state for v in row)
        assert len(b) == self.net.N ** 2
        return choice(Q1(self.net, b) if self.depth else Q0(self.net, b))


def check_move(ref):
    """move() above against the reference's Game2048._move (board and merged list)."""
    sys.path.insert(0, os.path.join(ref, "src"))
    from game2048 import Game2048

    rng = np.random.default_rng(1)
    for N in BOARD_SIZES:
        for _ in range(200):
            e = rng.integers(0, 6, size=N * N) * (rng.random(N * N) < 0.7)
            for a in range(4):
                g = Game2048(N)
                g.board = np.where(e > 0, 1 << e, 0).astype(np.int64).reshape(N, N)
                g._new_merged = []
                g._move(a)
                m, score = move(tuple(int(x) for x in e), N, a)
                assert tuple(exponents(g.board).tolist()) == m
                assert score == sum(int(v) for v in g._new_merged)


def is_dead(b, N):
    return all(move(b, N, a)[0] == b for a in range(4))


# --------------------------------------------------------------------------------------------------------- episodes
def record(E, RA, M, size, env_kw, fn, seeds_e, seeds_p, count, model_seed):
    """`count` episodes of the reference's run_episode with fn: per-episode fields, the boards before every step, the
    actions, the rewards and whether each episode's last step terminated it."""
    env = E.Game2048Env(E.Game2048EnvConfig(size=size, **env_kw))
    agent = RA.ReinforceAgent(env, M.MLPConfig(hidden_sizes=[8], activation="ReLU"), RA.ReinforceAgentConfig(model_seed=model_seed))
    steplog = []
    orig_sel = agent.select_action

    def sel(obs, rng, action_fn=None, use_greedy=False):
        steplog.append(exponents(agent.env.game.board))
        return orig_sel(obs, rng, action_fn, use_greedy)

    agent.select_action = sel
    ep = {k: [] for k in ("env_seed", "policy_seed", "length", "total_reward", "max_tile", "terminated")}
    acts, rews = [], []
    for _ in range(count):
        es, ps = next(seeds_e), next(seeds_p)
        before = len(steplog)
        traj = agent.run_episode(es, ps, action_gen=fn)
        final = tuple(int(x) for x in exponents(agent.env.game.board))
        again = agent.run_episode(es, ps ^ 0x5555, action_gen=fn)    # the policy stream is never drawn from
        del steplog[before + len(traj["actions"]):]
        assert again["actions"] == traj["actions"] and again["rewards"] == traj["rewards"]
        assert len(steplog) - before == len(traj["actions"])
        ep["env_seed"].append(es)
        ep["policy_seed"].append(ps)
        ep["length"].append(len(traj["actions"]))
        ep["total_reward"].append(traj["total_reward"])
        ep["max_tile"].append(traj["max_tile"])
        ep["terminated"].append(is_dead(final, size))
        acts += traj["actions"]
        rews += traj["rewards"]
    dt = dict(env_seed=np.uint64, policy_seed=np.uint64, length=np.int64, total_reward=np.float64, max_tile=np.int64,
              terminated=np.bool_)
    out = {k: np.array(v, dtype=dt[k]) for k, v in ep.items()}
    out["boards"] = np.stack(steplog).astype(np.uint8)
    out["actions"] = np.array(acts, dtype=np.uint8)
    out["rewards"] = np.array(rews, dtype=np.float64)
    assert int(out["boards"].max()) < 15
    return out


def gen_episodes(E, RA, M, nets, data):
    for c, case in enumerate(EP_CASES):
        fn = Player(nets[case["size"]], case["depth"])
        rec = record(E, RA, M, case["size"], case["env"], fn, seed_iter(17000 + c), seed_iter(18000 + c), EPISODES, c)
        for k, v in rec.items():
            data[f"e{c}_{k}"] = v
        print(f"  episodes {case['name']}: lengths {rec['length'].tolist()}, max tiles {rec['max_tile'].tolist()}",
              flush=True)


# ----------------------------------------------------------------------------------------------------------- boards
def gen_boards(nets, data):
    for N in BOARD_SIZES:
        rng = np.random.default_rng(900 + N)               # make_golden_search.py's boards
        boards = special_boards(N, rng)
        for i in range(N_RANDOM):
            fill = 0.3 + 0.7 * rng.random()
            top = int(rng.integers(3, 15))
            boards.append(rng.integers(1, top + 1, size=N * N) * (rng.random(N * N) < fill))
        boards = np.stack(boards).astype(np.uint8)
        tup = [tuple(int(x) for x in b) for b in boards]
        net = nets[N]
        data[f"b{N}_boards"] = boards
        data[f"b{N}_v"] = np.array([net.V(b) for b in tup], dtype=np.int64)
        q0 = np.array([Q0(net, b) for b in tup], dtype=np.int64)
        data[f"b{N}_q0"] = q0
        data[f"b{N}_a0"] = np.array([choice(r) for r in q0.tolist()], dtype=np.uint8)
        i1 = np.arange(0, len(tup), Q1_STEP[N])
        q1 = np.array([Q1(net, tup[i]) for i in i1], dtype=np.int64)
        data[f"b{N}_i1"] = i1.astype(np.int64)
        data[f"b{N}_q1"] = q1
        data[f"b{N}_a1"] = np.array([choice(r) for r in q1.tolist()], dtype=np.uint8)
        nvalid = (q0 != INVALID).sum(axis=1)
        ties = ((q0 == q0.max(axis=1, keepdims=True)) & (q0 != INVALID)).sum(axis=1) > 1
        neg = int(((q1 < 0) & (q1 != INVALID)).sum())
        assert (nvalid == 0).sum() >= 6 and (nvalid == 1).sum() >= 8 and ties.sum() >= 10, N
        print(f"  boards N={N}: {len(boards)} boards, {len(net.features)} features, {len(net.w)} weights, ties "
              f"{int(ties.sum())}, negative Q_1 {neg}, choices differ between depth 0 and 1 on "
              f"{int((data[f'b{N}_a0'][i1] != data[f'b{N}_a1']).sum())} of {len(i1)}", flush=True)


# --------------------------------------------------------------------------------------------------------------- TD
def gen_td(E, RA, M, nets, data):
    lr_num, lr_shift = TD_LR
    for N, env_kw in TD_CASES.items():
        net = nets[N]
        rec = record(E, RA, M, N, dict(R_RAW_MASK, **env_kw), Player(net, 0), seed_iter(19000 + N),
                     seed_iter(19500 + N), 6, N)
        acc = np.zeros(len(net.w), dtype=np.int64)
        rows = abs_delta = s = 0
        for L, term in zip(rec["length"].tolist(), rec["terminated"].tolist()):
            ms, gs = [], []
            for t in range(L):
                m, g = move(tuple(int(x) for x in rec["boards"][s + t]), N, int(rec["actions"][s + t]))
                ms.append(m)
                gs.append(g)
            vs = [net.V(m) for m in ms]
            for t in range(L):
                if t < L - 1:
                    y = (gs[t + 1] << F) + vs[t + 1]
                elif term:
                    y = 0
                else:
                    continue
                d = y - vs[t]
                step = max(-(1 << 30), min(1 << 30, (d * lr_num) >> lr_shift))
                np.add.at(acc, np.array(net.positions(ms[t]), dtype=np.int64), step)
                rows += 1
                abs_delta += abs(d)
            s += L
        new = (net.w.astype(np.int64) + acc).astype(np.uint64).astype(np.uint32).view(np.int32)   # wraps like np.int32
        pos = np.nonzero(new != net.w)[0]
        P = f"td{N}_"
        for k in ("env_seed", "policy_seed", "length", "terminated", "boards", "actions"):
            data[P + k] = rec[k]
        data[P + "lr"] = np.array(TD_LR, dtype=np.int64)
        data[P + "rows"] = np.int64(rows)
        data[P + "abs_delta"] = np.int64(abs_delta)
        data[P + "pos"] = pos.astype(np.int64)
        data[P + "val"] = (new[pos].astype(np.int64) - net.w[pos].astype(np.int64)).astype(np.int64)
        print(f"  td N={N}: lengths {rec['length'].tolist()}, terminated {rec['terminated'].tolist()}, rows {rows}, "
              f"sum |delta| {abs_delta}, {len(pos)} weights changed", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    E, RA, M = MR.import_reference(args.ref)
    check_move(args.ref)
    nets = {N: Net(N, HASH_SEED + N) for N in BOARD_SIZES}
    data = {"ep_cases": np.array(json.dumps(EP_CASES)), "frac_bits": np.int64(F),
            "hash_seed": np.array([HASH_SEED + N for N in range(9)], dtype=np.int64)}
    gen_boards(nets, data)
    gen_episodes(E, RA, M, nets, data)
    gen_td(E, RA, M, nets, data)
    out = os.path.join(HERE, "ntuple.npz")
    np.savez_compressed(out, **data)
    print("wrote", out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < (1 << 20), "committed files stay below 1 MiB"


if __name__ == "__main__":
    main()
