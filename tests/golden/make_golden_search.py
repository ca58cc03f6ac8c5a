"""Generate the expectimax-player fixtures from the REAL reference (build container only).

    python tests/golden/make_golden_search.py [--ref /root/reference]

Imports the reference the way make_golden_ref.py does and writes tests/golden/search.npz (data only).  The player is
written out here on its own (Player below: include/g2048_search.h's definition in plain Python, no project code), its
move is first checked against the reference's Game2048._move, and the reference plays it:

  episodes    e{c}_*: ReinforceAgent.run_episode(env_seed, policy_seed, action_gen=Player(...)), 2 episodes per case,
              in scripted.npz's per-case format (boards before each step as uint8 exponents [rows, N*N], actions, fp64
              rewards; per episode seeds, length, total_reward, max_tile).  Cases ("ep_cases", JSON, each with its
              depth): 4 x 4 depth 0 default config; 4 x 4 depth 1 on tests/rollout_replay.CONFIGS["R-raw-mask"] with
              max_steps 60; N = 3 depth 1 and depth 2 and N = 2 depth 2 on it with max_steps None; N = 5 depth 1 with
              max_steps 40; N = 8 depth 0 with max_steps 48; N = 3 depth 1 on CONFIGS["R-log2-nomask"] (mask off).
              Every episode is run a second time under another policy seed and must not differ.
  boards      b{N}_boards [m, N*N] uint8 exponents for N in 2, 3, 4, 5, 8 (m about 300: random fills 30-100 % with
              exponents up to 14, full boards, boards with one valid move, dead boards, transpose-symmetric boards that
              tie), b{N}_q{d} [m, 4] int64 (Q_d, -1 for an invalid action) and b{N}_a{d} [m] uint8 (the choice) for
              d = 0, 1; for N <= 4 also b{N}_i2 (about 40 board indices) with b{N}_q2 / b{N}_a2 at depth 2.
              Default weights (4, 16, 1, 2) throughout ("weights").
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

R_LOG2_NOMASK = dict(TERMS, reward_mode="sum", bonus_mode="log2", use_action_mask=False)
WEIGHTS = (4, 16, 1, 2)

EP_CASES = [
    dict(name="4x4-d0-default", size=4, depth=0, env=dict(max_steps=None)),
    dict(name="4x4-d1-terms-60", size=4, depth=1, env=dict(R_RAW_MASK, max_steps=60)),
    dict(name="3x3-d1-terms", size=3, depth=1, env=dict(R_RAW_MASK, max_steps=None)),
    dict(name="3x3-d2-terms", size=3, depth=2, env=dict(R_RAW_MASK, max_steps=None)),
    dict(name="2x2-d2-terms", size=2, depth=2, env=dict(R_RAW_MASK, max_steps=None)),
    dict(name="5x5-d1-terms-40", size=5, depth=1, env=dict(R_RAW_MASK, max_steps=40)),
    dict(name="8x8-d0-terms-48", size=8, depth=0, env=dict(R_RAW_MASK, max_steps=48)),
    dict(name="3x3-d1-nomask", size=3, depth=1, env=dict(R_LOG2_NOMASK, max_steps=None)),
]
EPISODES = 2
BOARD_SIZES = (2, 3, 4, 5, 8)
N_RANDOM, N_DEPTH2 = 240, 40


# ------------------------------------------------------------------------------------------------------- the player
def line_left(cells):
    out, gain, i, c = [], 0, 0, [x for x in cells if x]
    while i < len(c):
        if i + 1 < len(c) and c[i] == c[i + 1]:
            assert c[i] < 15, "a 2^15 + 2^15 merge is outside the pinned domain (the device saturates it)"
            out.append(c[i] + 1)
            gain += c[i] + 1
            i += 2
        else:
            out.append(c[i])
            i += 1
    return out + [0] * (len(cells) - len(out)), gain


def move(b, N, a):
    """b: tuple of N*N exponents, row-major; 0 up, 1 right, 2 down, 3 left -> (board, gain)."""
    nb, gain = list(b), 0
    for k in range(N):
        idx = [k * N + j for j in range(N)] if a in (3, 1) else [j * N + k for j in range(N)]
        if a in (1, 2):
            idx = idx[::-1]
        new, g = line_left([b[i] for i in idx])
        gain += g
        for i, v in zip(idx, new):
            nb[i] = v
    return tuple(nb), gain


def H(b, N, w):
    s = 0
    for r in range(N):
        for c in range(N):
            e = b[r * N + c]
            if c + 1 < N:
                s += 15 - abs(e - b[r * N + c + 1])
            if r + 1 < N:
                s += 15 - abs(e - b[(r + 1) * N + c])
    cg = sum(b[r * N + c] * ((N - 1 - r) + (N - 1 - c)) for r in range(N) for c in range(N))
    return w[1] * sum(1 for x in b if x == 0) + w[2] * s + w[3] * cg


def C(m, N, w, d):
    if d == 0:
        return H(m, N, w)
    tot = E = 0
    for c in range(N * N):
        if m[c] == 0:
            E += 1
            for k, p in ((1, 9), (2, 1)):
                nb = list(m)
                nb[c] = k
                tot += p * V(tuple(nb), N, w, d - 1)
    return tot // (10 * E)


def Q(b, N, w, d):
    qs = []
    for a in range(4):
        m, g = move(b, N, a)
        qs.append(-1 if m == b else w[0] * g + C(m, N, w, d))
    return qs


def V(b, N, w, d):
    return max([q for q in Q(b, N, w, d) if q >= 0], default=0)


def choice(qs):
    best = 0
    for a in range(4):
        if qs[a] > qs[best]:
            best = a
    return best


class Player:
    """action_gen for the reference's run_episode: (state, action_mask) -> action."""

    def __init__(self, N, depth, w=WEIGHTS):
        self.N, self.depth, self.w = N, depth, w

    def __call__(self, state, action_mask):
        b = tuple(int(v).bit_length() - 1 if v else 0 for row in state for v in row)
        assert len(b) == self.N * self.N
        return choice(Q(b, self.N, self.w, self.depth))


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
                m, gain = move(tuple(int(x) for x in e), N, a)
                assert tuple(exponents(g.board).tolist()) == m
                assert gain == sum(int(v).bit_length() - 1 for v in g._new_merged)


# --------------------------------------------------------------------------------------------------------- episodes
def gen_episodes(E, RA, M, data):
    mlp = M.MLPConfig(hidden_sizes=[8], activation="ReLU")
    for c, case in enumerate(EP_CASES):
        env = E.Game2048Env(E.Game2048EnvConfig(size=case["size"], **case["env"]))
        agent = RA.ReinforceAgent(env, mlp, RA.ReinforceAgentConfig(model_seed=c))
        fn = Player(case["size"], case["depth"])
        steplog = []
        orig_sel = agent.select_action

        def sel(obs, rng, action_fn=None, use_greedy=False, _o=orig_sel, _a=agent, _l=steplog):
            _l.append(exponents(_a.env.game.board))
            return _o(obs, rng, action_fn, use_greedy)

        agent.select_action = sel
        it_e, it_p = seed_iter(7000 + c), seed_iter(8000 + c)
        ep = {k: [] for k in ("env_seed", "policy_seed", "length", "total_reward", "max_tile")}
        acts, rews = [], []
        for _ in range(EPISODES):
            es, ps = next(it_e), next(it_p)
            before = len(steplog)
            traj = agent.run_episode(es, ps, action_gen=fn)
            again = agent.run_episode(es, ps ^ 0x5555, action_gen=fn)    # the policy stream is never drawn from
            del steplog[before + len(traj["actions"]):]
            assert again["actions"] == traj["actions"] and again["rewards"] == traj["rewards"]
            assert len(steplog) - before == len(traj["actions"])
            ep["env_seed"].append(es)
            ep["policy_seed"].append(ps)
            ep["length"].append(len(traj["actions"]))
            ep["total_reward"].append(traj["total_reward"])
            ep["max_tile"].append(traj["max_tile"])
            acts += traj["actions"]
            rews += traj["rewards"]
        P = f"e{c}_"
        dt = dict(env_seed=np.uint64, policy_seed=np.uint64, length=np.int64, total_reward=np.float64, max_tile=np.int64)
        for k, v in ep.items():
            data[P + k] = np.array(v, dtype=dt[k])
        data[P + "boards"] = np.stack(steplog).astype(np.uint8)
        data[P + "actions"] = np.array(acts, dtype=np.uint8)
        data[P + "rewards"] = np.array(rews, dtype=np.float64)
        assert int(data[P + "boards"].max()) < 15
        print(f"  episodes {case['name']}: lengths {ep['length']}, max tiles {ep['max_tile']}", flush=True)


# ----------------------------------------------------------------------------------------------------------- boards
def dead_board(N, rng):
    """No empty cell and no equal neighbours: two interleaved sets of exponents on a checkerboard."""
    lo, hi = rng.integers(1, 8, size=N * N), rng.integers(8, 15, size=N * N)
    return np.array([(lo if (k // N + k % N) & 1 else hi)[k] for k in range(N * N)])


def special_boards(N, rng):
    out = []
    for _ in range(10):                                  # full boards (some with a merge available)
        out.append(rng.integers(1, 7, size=N * N))
    for _ in range(6):
        out.append(dead_board(N, rng))
    for k in range(8):                                   # one valid move: an empty edge column / row on a dead board
        b = dead_board(N, rng).reshape(N, N)
        if k % 4 == 0:
            b[:, N - 1] = 0
        elif k % 4 == 1:
            b[:, 0] = 0
        elif k % 4 == 2:
            b[N - 1, :] = 0
        else:
            b[0, :] = 0
        out.append(b.reshape(-1))
    for _ in range(30):                                  # transpose-symmetric: up ties with left, right with down
        b = (rng.integers(0, 8, size=(N, N)) * (rng.random((N, N)) < 0.7))
        b = np.triu(b) + np.triu(b, 1).T
        out.append(b.reshape(-1))
    return out


def gen_boards(data):
    for N in BOARD_SIZES:
        rng = np.random.default_rng(900 + N)
        boards = special_boards(N, rng)
        for i in range(N_RANDOM):
            fill = 0.3 + 0.7 * rng.random()
            top = int(rng.integers(3, 15))
            boards.append(rng.integers(1, top + 1, size=N * N) * (rng.random(N * N) < fill))
        boards = np.stack(boards).astype(np.uint8)
        tup = [tuple(int(x) for x in b) for b in boards]
        data[f"b{N}_boards"] = boards
        stats = {}
        for d in (0, 1):
            q = np.array([Q(b, N, WEIGHTS, d) for b in tup], dtype=np.int64)
            data[f"b{N}_q{d}"] = q
            data[f"b{N}_a{d}"] = np.array([choice(list(r)) for r in q], dtype=np.uint8)
            nvalid = (q >= 0).sum(axis=1)
            ties = ((q == q.max(axis=1, keepdims=True)) & (q >= 0)).sum(axis=1) > 1
            stats[d] = dict(dead=int((nvalid == 0).sum()), one=int((nvalid == 1).sum()), ties=int(ties.sum()))
            assert stats[d]["dead"] >= 6 and stats[d]["one"] >= 8 and stats[d]["ties"] >= 10, (N, d, stats[d])
        full = int((boards != 0).all(axis=1).sum())
        assert full >= 16 and int(boards.max()) == 14
        if N <= 4:
            i2 = np.concatenate([np.arange(0, 54, 3), 54 + rng.choice(N_RANDOM, N_DEPTH2 - 18, replace=False)])
            q = np.array([Q(tup[i], N, WEIGHTS, 2) for i in i2], dtype=np.int64)
            data[f"b{N}_i2"] = i2.astype(np.int64)
            data[f"b{N}_q2"] = q
            data[f"b{N}_a2"] = np.array([choice(list(r)) for r in q], dtype=np.uint8)
        print(f"  boards N={N}: {len(boards)} boards, {full} full, depth 0 {stats[0]}, depth 1 {stats[1]}, "
              f"choices differ between depth 0 and 1 on {int((data[f'b{N}_a0'] != data[f'b{N}_a1']).sum())}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    E, RA, M = MR.import_reference(args.ref)
    check_move(args.ref)
    data = {"ep_cases": np.array(json.dumps(EP_CASES)), "weights": np.array(WEIGHTS, dtype=np.int64)}
    gen_boards(data)
    gen_episodes(E, RA, M, data)
    out = os.path.join(HERE, "search.npz")
    np.savez_compressed(out, **data)
    print("wrote", out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < (1 << 20), "committed files stay below 1 MiB"


if __name__ == "__main__":
    main()
