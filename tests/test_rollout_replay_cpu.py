"""CPU: tests/rollout_replay.py pinned to what it restates, and shown able to fail.

* the vectorised choice equals numpy's Generator.choice(4, p=...) on 12,000 fp32 masked-softmax rows;
* replay_4x4 passes a batch played lane by lane in the per-lane oracle (oracle.Env) and fails after each single
  corruption of it; the same for replay_sized at N = 3 and 6 on batches played in SizedRef;
* SizedRef(4, cfg) equals oracle.Env(**cfg) on every field under the four env configs of the replay tests
  (bonus_mode="raw" included), which ties the two checkers to each other under those configs.
"""
import copy
import types

import numpy as np
import pytest

import rollout_replay as RR
import sized_ref as SR
from oracle import oracle as O

FULL = dict(RR.CONFIGS["S-raw-nomask"], max_steps=200)         # every term, no action mask
N_EP = 70


# ------------------------------------------------------------------------------------------------------- 1. choice
def _softmax32(logits, mask):
    """logits_to_probs in fp32: where(mask, logits, -1e9), max-shifted."""
    l = np.where(mask, logits, np.float32(-1e9)).astype(np.float32)
    e = np.exp(l - l.max(axis=1, keepdims=True), dtype=np.float32)
    return (e / e.sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)


def test_vectorised_choice_equals_generator_choice():
    g = np.random.default_rng(2048)
    episodes, rows = 240, 50
    m = episodes * rows
    logits = (g.standard_normal((m, 4)) * g.choice([0.3, 1.0, 4.0], size=(m, 1))).astype(np.float32)
    near_one = np.arange(m) % 7 == 0
    logits[near_one, g.integers(4, size=int(near_one.sum()))] += np.float32(20.0)
    mask = np.ones((m, 4), dtype=bool)
    n_masked = np.arange(m) % 4                                   # 0, 1, 2, 3 masked entries in turn
    for r in range(m):
        mask[r, g.permutation(4)[:n_masked[r]]] = False
    p = _softmax32(logits, mask)
    assert p.dtype == np.float32 and bool((p[~mask] == 0.0).all())
    assert all(int(((~mask).sum(axis=1) == k).sum()) >= 1000 for k in (1, 2, 3))
    top = p.max(axis=1)
    assert int(((top >= 1 - 1e-6) & (top <= 1.0)).sum()) >= 1000
    assert int((top < 0.9).sum()) >= 1000
    want = np.zeros(m, dtype=np.int64)
    u = np.zeros(m)
    for e in range(episodes):
        seed = 5_000_000 + e
        u[e * rows:(e + 1) * rows] = np.random.default_rng(seed).random(rows)
        pol = np.random.default_rng(seed)
        want[e * rows:(e + 1) * rows] = [int(pol.choice(4, p=p[r])) for r in range(e * rows, (e + 1) * rows)]
    got = RR.choice4(p, u)
    assert int((got != want).sum()) == 0
    assert len(np.unique(want)) == 4 and bool(mask[np.arange(m), want].all())
    # and through check_choices, in the batch layout: [T, n] with ragged lengths
    T, n = rows, episodes
    lengths = 1 + (np.arange(n) * 7) % rows
    lengths[0] = rows
    probs = p.reshape(n, T, 4).transpose(1, 0, 2).copy()
    acts = want.reshape(n, T).T.astype(np.uint8).copy()
    seeds = 5_000_000 + np.arange(n)
    assert RR.check_choices(probs, acts, lengths, seeds, False, None) == int(lengths.sum())
    bad = acts.copy()
    bad[0, 3] = (bad[0, 3] + 1) % 4
    with pytest.raises(AssertionError, match="choice"):
        RR.check_choices(probs, bad, lengths, seeds, False, None)
    # greedy: the first maximum of p * mask
    bits = (mask.reshape(n, T, 4).transpose(1, 0, 2) << np.arange(4)).sum(axis=2).astype(np.uint8)
    first = (probs * mask.reshape(n, T, 4).transpose(1, 0, 2)).argmax(axis=2).astype(np.uint8)
    assert RR.check_choices(probs, first, lengths, seeds, True, bits) == int(lengths.sum())
    with pytest.raises(AssertionError, match="choice"):
        RR.check_choices(probs, bad, lengths, seeds, True, bits)


# ------------------------------------------------------------------------------------- 2. synthetic batches to replay
def _flags(r):
    from rl2048_amd import _lib as L

    return ((L.F_CHANGED if r["changed"] else 0) | (L.F_TERMINATED if r["terminated"] else 0) |
            (L.F_TRUNCATED if r["truncated"] else 0) | (L.F_INVALID if r["invalid"] else 0))


def _batch(episodes, words, planes):
    """episodes: per episode (rows of (board words, action, reward, flags), max tile, final board words)."""
    from rl2048_amd import _lib as L

    n, T = len(episodes), max(len(rows) for rows, _, _ in episodes)
    boards = np.zeros((words, T, n), dtype=np.uint64)
    actions = np.zeros((T, n), dtype=np.uint8)
    rewards = np.zeros((T, n), dtype=np.float64)
    flags = np.full((T, n), L.F_INACTIVE, dtype=np.uint8)
    final = np.zeros((words, n), dtype=np.uint64)
    total = np.zeros(n, dtype=np.float64)
    for i, (rows, _, fb) in enumerate(episodes):
        for t, (b, a, r, f) in enumerate(rows):
            boards[:, t, i], actions[t, i], rewards[t, i], flags[t, i] = b, a, r, f
            total[i] += r                                   # step order
        final[:, i] = fb
    sq = (lambda x: x) if planes else (lambda x: x[0])         # sized batches keep the plane axis, W = 1 included
    return types.SimpleNamespace(boards=sq(boards).view(np.int64), actions=actions, rewards=rewards, flags=flags,
                                 lengths=np.array([len(rows) for rows, _, _ in episodes], dtype=np.int32),
                                 total_reward=total, max_tile=np.array([m for _, m, _ in episodes], dtype=np.int64),
                                 final_boards=sq(final).view(np.int64), probs=None)


def _play_4x4(seeds, cfg=FULL):
    g = np.random.default_rng(11)
    pack = lambda e: [O.pack_exponents(O.values_to_exponents(e.board))]
    episodes = []
    for s in seeds:
        e = O.Env(**cfg)
        e.reset(int(s))
        rows = []
        while True:
            b, a = pack(e), int(g.integers(4))
            r = e.step(a)
            rows.append((b, a, r["reward"], _flags(r)))
            if r["terminated"] or r["truncated"]:
                break
        episodes.append((rows, e.max_tile_seen, pack(e)))
    return _batch(episodes, 1, planes=False)


def _play_sized(size, seeds):
    g = np.random.default_rng(12 + size)
    pack = lambda e: SR.pack_planes(SR.exponents(e.board).reshape(1, -1), size)[:, 0].view(np.uint64)
    episodes = []
    for s in seeds:
        e = SR.SizedRef(size, FULL)
        e.reset(int(s))
        rows = []
        while True:
            b, a = pack(e), int(g.integers(4))
            r = e.step(a)
            rows.append((b, a, r["reward"], _flags(r)))
            if r["terminated"] or r["truncated"]:
                break
        episodes.append((rows, e.max_tile_seen, pack(e)))
    return _batch(episodes, SR.words(size), planes=True)


def _reward_ulp(b):
    t = int(b.lengths[1]) // 2
    b.rewards[t, 1] = np.nextafter(b.rewards[t, 1], np.inf)


def _max_tile_doubled(b):
    b.max_tile[2] *= 2


def _total_reversed(b):
    rev = np.zeros_like(b.total_reward)
    for t in range(b.actions.shape[0] - 1, -1, -1):
        rev += np.where(t < b.lengths, b.rewards[t], 0.0)
    differs = rev.view(np.uint64) != b.total_reward.view(np.uint64)
    assert differs.any(), "the reversed sum has the same bits in every episode: this corruption shows nothing"
    b.total_reward[:] = rev


def _length_shortened(b):
    i = int(np.argmin(b.lengths))               # not the longest: T stays lengths.max()
    assert b.lengths[i] > 1
    b.lengths[i] -= 1


def _board_nibble(b):
    from rl2048_amd import _lib as L

    t = int(b.lengths[3]) - 1
    assert not b.flags[t, 3] & L.F_INACTIVE
    plane = b.boards if b.boards.ndim == 2 else b.boards[0]
    plane[t, 3] ^= np.int64(1) << np.int64(4 * 2)


def _invalid_cleared(b):
    from rl2048_amd import _lib as L

    valid = np.arange(b.actions.shape[0])[:, None] < b.lengths[None, :]
    t, i = (x[0] for x in np.nonzero(valid & ((b.flags & L.F_INVALID) != 0)))
    b.flags[t, i] &= np.uint8(0xFF ^ L.F_INVALID)


CORRUPTIONS = [(_reward_ulp, "rewards"), (_max_tile_doubled, "max_tile"), (_total_reversed, "total_reward"),
               (_length_shortened, "episode end"), (_board_nibble, "boards"), (_invalid_cleared, "flags")]


def _passes_and_fails(batch, replay):
    c = replay(batch)
    assert c["rows"] == int(batch.lengths.sum())
    assert c["terminated"] + c["truncated"] == N_EP
    assert c["invalid"] > 0 and c["merges"] > 0 and c["bonus"] > 0 and c["changed"] > 0
    for corrupt, what in CORRUPTIONS:
        bad = copy.deepcopy(batch)
        corrupt(bad)
        with pytest.raises(AssertionError, match=what):
            replay(bad)
    return c


def test_replay_4x4_equals_the_per_lane_oracle_and_can_fail():
    """n = 70 episodes of random play in oracle.Env under the full-term config without action mask, max_steps 200."""
    seeds = np.arange(810_000, 810_000 + N_EP)
    batch = _play_4x4(seeds)
    c = _passes_and_fails(batch, lambda b: RR.replay_4x4(b, FULL, seeds))
    assert c["terminated"] > 0 and c["truncated"] > 0
    assert c["masks"] is None           # no action mask in this config
    # with the mask on the replay also returns the oracle's mask of every recorded board
    on = dict(FULL, use_action_mask=True)
    few = seeds[:6]
    b2 = _play_4x4(few, on)
    masks = RR.replay_4x4(b2, on, few)["masks"]
    for i, s in enumerate(few):
        e = O.Env(**on)
        e.reset(int(s))
        for t in range(int(b2.lengths[i])):
            assert masks[t, i] == SR.mask_bits(e.mask()), (i, t)
            e.step(int(b2.actions[t, i]))
        assert not masks[int(b2.lengths[i]):, i].any()


@pytest.mark.parametrize("size", [3, 6])
def test_replay_sized_equals_sized_ref_and_can_fail(size):
    seeds = np.arange(820_000, 820_000 + N_EP)
    batch = _play_sized(size, seeds)
    c = _passes_and_fails(batch, lambda b: RR.replay_sized(b, size, FULL, seeds))
    assert (c["terminated"] if size == 3 else c["truncated"]) == N_EP


# ------------------------------------------------------------------------------------ 3. the two checkers, each other
@pytest.mark.parametrize("name", list(RR.CONFIGS))
def test_sized_ref_at_4_equals_the_oracle_env(name):
    """50 seeded episodes per config, obs mode in turn: every step's reward (fp64 bits), changed / terminated /
    truncated / invalid, and after it the board, max_tile_seen, score, step count, obs and mask.  With the mask on the
    actions are drawn from the valid ones, as a masked policy does."""
    g = np.random.default_rng(len(name))
    ends = dict(terminated=0, truncated=0, invalid=0, bonus=0)
    for k in range(50):
        cfg = dict(RR.CONFIGS[name], obs_mode=("log2", "raw", "onehot")[k % 3], max_steps=150)
        a, b = O.Env(**cfg), SR.SizedRef(4, cfg)
        a.reset(930_000 + k)
        b.reset(930_000 + k)
        while True:
            np.testing.assert_array_equal(a.board, b.board)
            np.testing.assert_array_equal(a.mask(), b.mask())
            np.testing.assert_array_equal(a.obs(), b.obs().reshape(-1))
            assert (a.max_tile_seen, a.score, a.step_count) == (b.max_tile_seen, b.score, b.steps)
            valid = np.nonzero(a.mask())[0]
            act = int(g.choice(valid)) if cfg["use_action_mask"] else int(g.integers(4))
            seen = a.max_tile_seen
            ra, rb = a.step(act), b.step(act)
            assert np.float64(ra["reward"]).view(np.uint64) == np.float64(rb["reward"]).view(np.uint64), (k, ra, rb)
            for f in ("changed", "terminated", "truncated", "invalid"):
                assert ra[f] == rb[f], (k, f)
                ends[f] = ends.get(f, 0) + int(ra[f])
            ends["bonus"] += int(a.max_tile_seen > seen)
            if ra["terminated"] or ra["truncated"]:
                break
        np.testing.assert_array_equal(a.board, b.board)
        assert a.max_tile_seen == b.max_tile_seen
    assert ends["terminated"] > 0 and ends["truncated"] > 0 and ends["bonus"] > 0
    assert (ends["invalid"] > 0) == (not RR.CONFIGS[name]["use_action_mask"])
