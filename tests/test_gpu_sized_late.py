"""GPU parity of the sized (2..8) env kernels on dense, late-game and high-tile boards: the states random play from
reset (tests/golden/sized.npz, tests/test_gpu_sized.py) never reaches within its 60 recorded steps.

  a. the episodes of tests/golden/sized_late.npz -- the REAL reference started on injected late-game boards
     (tests/golden/make_golden_sized_late.py) -- replayed through VecGame2048Env at every size, N = 4 through the sized
     entry points;
  b. a bulk differential against tests/sized_ref.py (a plain NumPy game + env, pinned to the reference on those very
     states by tests/test_sized_ref_cpu.py): 1031 lanes of family boards, random actions, planted max_tile_seen and
     step counts, and the whole PCG64 state after every step;
  c. the Lemire rejection fallback of the spawn on sized boards (a planted buffered uint32);
  d. auto-reset after *termination*, PCG64 and Philox, against a fresh reset(seed + stride) of the reference
     implementation; live Philox lanes against the exact spawn rule;
  e. g2048_sized_move / _obs / _symmetries on their own outputs, at every size, with padded plane strides.

Every comparison is equality; the fp32 reward is np.float32(the fp64 reference reward).  On a step whose merge
saturates (2^15 + 2^15) the expected board is the reference's clipped to 2^15, F_OVERFLOW is expected there and
nowhere else, and done / mask / obs are those of the clipped board (sized_ref.SizedRef
saturate=True, which test_sized_ref_cpu.py shows to differ from the reference in nothing else).

What a wrong kernel would trip here while tests/test_gpu_sized.py stays green (its boards hold exponents <= 6 and at
least 7 empty cells at N >= 5, and never end):
  * a line move that drops nibble bit 3 (v & 7): every tile of 2^8 and above -- a, b, e at every size;
  * spawn_pcg drawing for one empty cell: a move on a hole* board leaves exactly one empty cell again, and b
    compares rng_state / rng_uint / LS_HAS_U32 after that very step (the board alone would not show it);
  * is_done or the action mask skipping a word, or the shifted-in neighbour of a word's first nibble: the
    checkerboards and pair_row / pair_col boards are full, so done and the mask hang on every cell, the last word's
    included; the holes sit in the first and last nibble of each word;
  * a merged list that stops short, or a count that wraps: all1 / all14 / all15 / eq_rows / eq_cols fill all
    N * (N // 2) slots (sized.npz: at most 6 of up to 32);
  * a store or load with the wrong plane stride: e passes strides above the lane count and checks the pad columns;
  * the reset branch inside the step taking the old stream, seed or state word: d compares all of them with a fresh
    reset(seed + stride) after a *termination*.
A dropped cross-word or_row spill or a kth_empty off by one word already fails on sized.npz (early-game tiles do
reach the straddling rows and the second word); here the line* boards put 14 / 15 runs across every word boundary.
"""
import json
import os

import numpy as np
import pytest
import torch

import sized_ref as SR
from sized_ref import pack_planes, unpack_planes, words

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ALL_SIZES = [2, 3, 4, 5, 6, 7, 8]


@pytest.fixture(scope="module")
def lib():
    from rl2048_amd import _lib

    _lib.ensure_device(DEV)
    return _lib


@pytest.fixture(scope="module")
def late(golden_dir):
    with np.load(os.path.join(golden_dir, "sized_late.npz")) as z:
        return {k: z[k] for k in z.files}


def _env(n, kw, lanes, **opts):
    """A VecGame2048Env of size n; N = 4 re-pointed at the sized entry points."""
    from rl2048_amd import Game2048EnvConfig, VecGame2048Env

    env = VecGame2048Env(lanes, Game2048EnvConfig(size=n, **kw), device=DEV, **opts)
    return SR.as_sized4(env) if n == 4 else env


def _put_boards(env, e, n):
    env.board.copy_(torch.from_numpy(pack_planes(e, n)).to(DEV).view_as(env.board))


def _ow(n, mode):
    return n * n * (17 if mode == "onehot" else 1)


def _mask4(bits):
    return ((np.asarray(bits)[..., None] >> np.arange(4)) & 1).astype(np.int8)


# -------------------------------------------------------------------------------------------- a. fixture replay
_EXPECT: dict = {}


def _late_expect(late, n, c):
    """The fixture's step records of (n, c) as the kernels must report them: boards clipped to 2^15, and on a
    saturating step done / truncated / mask / reward of the clipped board (sized_ref, saturate=True)."""
    if (n, c) in _EXPECT:
        return _EXPECT[(n, c)]
    kw = json.loads(str(late["env_cfgs"]))[str(c)]
    p = f"n{n}_c{c}_"
    x = {k: late[p + k].copy() for k in ("board", "reward", "terminated", "truncated", "invalid", "max_tile_seen",
                                          "score", "step_index", "mask", "merged")}
    x["overflow"] = (x["merged"] == 16).any(axis=1)
    for e in np.flatnonzero(late[p + "ep_sat"]):
        start, ln = int(late[p + "ep_start"][e]), int(late[p + "ep_len"][e])
        ref = SR.SizedRef(n, kw, saturate=True)
        ref.reset(int(late[p + "ep_seed"][e]))
        ref.inject(SR.values(late[p + "ep_board"][e]))
        for j in range(start, start + ln):
            r = ref.step(int(late[p + "action"][j]))
        assert r["saturated"] and x["overflow"][j] and not x["overflow"][start:j].any()
        x["terminated"][j], x["truncated"][j], x["reward"][j] = r["terminated"], r["truncated"], r["reward"]
        x["mask"][j] = SR.mask_bits(ref.mask())
    x["board"] = np.minimum(x["board"], 15)
    x["obs"] = SR.obs_of(SR.values(x["board"]).reshape(-1, n, n), kw.get("obs_mode", "raw"),
                         kw.get("obs_log2_scale", 1.0))
    _EXPECT[(n, c)] = x
    return x


@pytest.mark.parametrize("lanes", [63, 1031])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
@pytest.mark.parametrize("n", ALL_SIZES)
def test_late_episodes_from_injected_boards(late, lib, n, c, lanes):
    kw = json.loads(str(late["env_cfgs"]))[str(c)]
    p = f"n{n}_c{c}_"
    x = _late_expect(late, n, c)
    seeds, starts, lens = late[p + "ep_seed"], late[p + "ep_start"].astype(int), late[p + "ep_len"].astype(int)
    E, T, W, LEN = len(seeds), int(lens.max()), words(n), n * (n // 2)
    ep = np.arange(lanes) % E
    env = _env(n, kw, lanes, record_merged=True)
    envp = _env(n, kw, lanes, packed_mask=True)                           # the packed action-mask form
    lane_seeds = [int(seeds[e]) for e in ep]
    env.reset(seed=lane_seeds)
    envp.reset(seed=lane_seeds)
    for v in (env, envp):
        _put_boards(v, late[p + "ep_board"][ep], n)
    mode = kw.get("obs_mode", "raw")
    OW = _ow(n, mode)
    acts = np.zeros((T, lanes), dtype=np.uint8)
    valid = np.zeros((T, lanes), dtype=bool)
    idx = np.zeros((T, lanes), dtype=np.int64)
    for i, e in enumerate(ep):
        acts[:lens[e], i] = late[p + "action"][starts[e]:starts[e] + lens[e]]
        valid[:lens[e], i] = True
        idx[:lens[e], i] = np.arange(starts[e], starts[e] + lens[e])
    # an episode the generator stopped (saturated, or 24 steps long) leaves its lane in mid-game: the lane is retired
    # by hand after its last step, so that every lane past its end must report F_INACTIVE
    last = np.zeros((T, lanes), dtype=bool)
    last[lens[ep] - 1, np.arange(lanes)] = True
    acts_d, last_d = torch.from_numpy(acts).to(DEV), torch.from_numpy(last).to(DEV)
    traj = torch.zeros(W, T, lanes, dtype=torch.int64, device=DEV)        # prev_board rows, plane stride T * lanes
    rew32 = torch.zeros(T, lanes, dtype=torch.float32, device=DEV)
    rew64 = torch.zeros(T, lanes, dtype=torch.float64, device=DEV)
    flags = torch.zeros(T, lanes, dtype=torch.uint8, device=DEV)
    flagsp = torch.zeros(T, lanes, dtype=torch.uint8, device=DEV)
    rec = {k: [] for k in ("board", "obs", "mask", "merged", "state", "score", "boardp", "bits", "obsp")}
    for t in range(T):
        env.step_into(acts_d[t], reward=rew32[t], flags=flags[t], prev_board=traj[:, t], reward64=rew64[t])
        envp.step_into(acts_d[t], flags=flagsp[t])
        rec["board"].append(env.board.clone().view(W, lanes))
        rec["obs"].append(env.obs.clone())
        rec["mask"].append(env.mask.clone())
        rec["merged"].append(env.merged.clone())
        rec["state"].append(env.state.clone())
        rec["score"].append(env.score.clone())
        rec["boardp"].append(envp.board.clone().view(W, lanes))
        rec["bits"].append(envp.mask_bits.clone())
        rec["obsp"].append(envp.obs.clone())
        for v in (env, envp):
            v.set_lane_state(active=v.active & ~last_d[t])
    h = {k: torch.stack(s).cpu().numpy() for k, s in rec.items()}
    fl, v = flags.cpu().numpy(), valid
    g = lambda k: x[k][idx]                                               # noqa: E731  [T, lanes, ...]
    assert np.array_equal(unpack_planes(np.moveaxis(h["board"], 1, 0), n)[v], g("board")[v])
    assert np.array_equal(rew64.cpu().numpy()[v].view(np.uint64), g("reward")[v].view(np.uint64))
    assert np.array_equal(rew32.cpu().numpy()[v], g("reward").astype(np.float32)[v])
    assert np.array_equal(((fl & lib.F_TERMINATED) != 0)[v], g("terminated")[v])
    assert np.array_equal(((fl & lib.F_TRUNCATED) != 0)[v], g("truncated")[v])
    assert np.array_equal(((fl & lib.F_INVALID) != 0)[v], g("invalid")[v])
    assert np.array_equal(((fl & lib.F_OVERFLOW) != 0)[v], g("overflow")[v])          # there and nowhere else
    assert (fl[~v] == lib.F_INACTIVE).all() and not (fl[v] & (lib.F_INACTIVE | lib.F_BADACTION | lib.F_RESET)).any()
    st = h["state"].view(np.uint32)
    assert np.array_equal((np.int64(1) << ((st >> 20) & 31).astype(np.int64))[v], g("max_tile_seen")[v])
    assert np.array_equal((st & 0xFFFFF).astype(np.int64)[v], g("step_index")[v])
    assert np.array_equal(h["score"][v], g("score")[v])
    gm = g("mask")
    assert np.array_equal(h["mask"][v], _mask4(gm)[v])
    assert np.array_equal(h["bits"][v], gm[v])
    assert np.array_equal(h["obs"].reshape(T, lanes, OW)[v], g("obs")[v])
    assert np.array_equal(h["obsp"].reshape(T, lanes, OW)[v], g("obs")[v])
    assert np.array_equal(h["merged"][v], g("merged")[v]) and h["merged"].shape == (T, lanes, LEN)
    assert np.array_equal(h["boardp"], h["board"]) and np.array_equal(flagsp.cpu().numpy(), fl)
    prev = unpack_planes(traj.cpu().numpy(), n)                           # [T, lanes, N*N]: the board before step t
    want_prev = np.concatenate([late[p + "ep_board"][ep][None], g("board")[:-1]])
    assert np.array_equal(prev[v], want_prev[v])
    # what the fixture is there for is in what was compared (test_sized_ref_cpu.py asserts it of the whole file)
    assert g("terminated")[v].any() and g("overflow")[v].any() and (g("merged")[v] == 15).any()


# ------------------------------------------------------------------------------------- b. bulk differential
def _rng_of(env):
    """(state, inc, uinteger, has_uint32) per lane as Python ints / arrays."""
    s = env.rng_state.cpu().numpy().view(np.uint64).reshape(-1, 2)
    c = env.rng_inc.cpu().numpy().view(np.uint64).reshape(-1, 2)
    state = [int(lo) | (int(hi) << 64) for lo, hi in s]
    inc = [int(lo) | (int(hi) << 64) for lo, hi in c]
    has = (env.state.cpu().numpy().view(np.uint32) & 0x04000000) != 0
    return state, inc, env.rng_uint.cpu().numpy().view(np.uint32), has


def _assert_rng(env, refs, lanes, where):
    state, inc, uint, has = _rng_of(env)
    for i in lanes:
        r = refs[i].rng_state
        assert (state[i], inc[i], int(uint[i]), int(has[i])) == (r["state"], r["inc"], r["uinteger"],
                                                                   r["has_uint32"]), (where, i)


def _plant_lane_state(env, maxt, stepc):
    mt = env.max_tile.cpu().numpy()
    sc = env.step_count.cpu().numpy()
    env.set_lane_state(step_count=torch.from_numpy(np.where(stepc >= 0, stepc, sc).astype(np.int32)),
                       max_tile_exp=torch.from_numpy(np.where(maxt > 0, maxt, mt).astype(np.int32)))


def _check_step(lib, n, env, envp, refs, live, acts, prev_exp, where):
    """Step the reference lanes in `live` by acts and compare everything the env reports.  Returns the step dicts."""
    cfg = refs[0].cfg
    L = env.n
    fl, flp = env.flags.cpu().numpy(), envp.flags.cpu().numpy()
    board = unpack_planes(env.board.cpu().numpy().reshape(words(n), L), n)
    boardp = unpack_planes(envp.board.cpu().numpy().reshape(words(n), L), n)
    prev = unpack_planes(env.prev_board.cpu().numpy().reshape(words(n), L), n)
    r32, r64 = env.reward.cpu().numpy(), env.reward64.cpu().numpy()
    mask, bits = env.mask.cpu().numpy(), envp.mask_bits.cpu().numpy()
    obs, obsp = env.obs.cpu().numpy(), envp.obs.cpu().numpy()
    merged, score = env.merged.cpu().numpy(), env.score.cpu().numpy()
    st = env.state.cpu().numpy().view(np.uint32)
    out = {}
    for i in live:
        w = (where, int(i))
        r = refs[i].step(int(acts[i]))
        out[i] = r
        want = (lib.F_CHANGED * r["changed"]) | (lib.F_TERMINATED * r["terminated"]) | \
            (lib.F_TRUNCATED * r["truncated"]) | (lib.F_INVALID * r["invalid"]) | (lib.F_OVERFLOW * r["saturated"])
        assert fl[i] == want and flp[i] == want, (w, fl[i], want)
        e = SR.exponents(refs[i].board).reshape(-1)
        assert np.array_equal(board[i], e) and np.array_equal(boardp[i], e), w
        assert np.array_equal(prev[i], prev_exp[i]), w
        assert r64[i] == r["reward"] and r32[i] == np.float32(r["reward"]), (w, r64[i], r["reward"])
        m = refs[i].mask()
        assert mask[i].tolist() == m and int(bits[i]) == SR.mask_bits(m), w
        o = refs[i].obs()
        assert np.array_equal(obs[i], o) and np.array_equal(obsp[i], o), w
        assert np.array_equal(merged[i], SR.pad_merged(r["merged"], n)), w
        assert int(score[i]) == r["score"], w
        assert int(st[i] & 0xFFFFF) == r["step_index"] and 1 << int((st[i] >> 20) & 31) == r["max_tile_seen"], w
        assert bool(st[i] & 0x02000000) == (not (r["terminated"] or r["truncated"])), w
    return out


@pytest.mark.parametrize("cfg_name", sorted(SR.BULK_CFGS))
@pytest.mark.parametrize("n", [2, 3, 5, 6, 7, 8])
def test_bulk_differential(lib, n, cfg_name):
    kw = SR.BULK_CFGS[cfg_name]
    refs, boards, seeds, actions, maxt, stepc = SR.bulk_refs(n, cfg_name)
    L = SR.BULK_LANES
    env = _env(n, kw, L, record_merged=True, record_prev_board=True, record_reward64=True)
    envp = _env(n, kw, L, packed_mask=True)
    for v in (env, envp):
        v.reset(seed=seeds)
        _put_boards(v, boards, n)
        _plant_lane_state(v, maxt, stepc)
    _assert_rng(env, refs, range(L), "reset")
    live = np.ones(L, dtype=bool)
    ended = np.zeros(L, dtype=bool)
    prev_exp = boards.copy()
    count = dict(saturated=0, terminated=0, truncated=0, invalid=0, bonus=0)
    for t in range(SR.BULK_STEPS):
        a = torch.from_numpy(actions[t]).to(DEV)
        env.step_into(a)
        envp.step_into(a)
        seen_before = {i: refs[i].max_tile_seen for i in np.flatnonzero(live)}
        res = _check_step(lib, n, env, envp, refs, np.flatnonzero(live), actions[t], prev_exp, (n, cfg_name, t))
        _assert_rng(env, refs, np.flatnonzero(live), (n, cfg_name, t))
        fl = env.flags.cpu().numpy()
        assert (fl[ended] == lib.F_INACTIVE).all() and not env.reward.cpu().numpy()[ended].any()
        for i, r in res.items():
            prev_exp[i] = SR.exponents(refs[i].board).reshape(-1)
            for k in ("saturated", "terminated", "truncated", "invalid"):
                count[k] += r[k]
            count["bonus"] += r["max_tile_seen"] > seen_before[i]
            if r["terminated"] or r["truncated"]:
                ended[i] = True
            if r["saturated"] or r["terminated"] or r["truncated"]:
                live[i] = False                       # a saturated lane is compared on that step, then dropped
    assert count["saturated"] <= L // 4 and min(count[k] for k in ("saturated", "terminated", "invalid", "bonus")) >= 1
    assert (count["truncated"] >= L // 6) == (kw["max_steps"] is not None), count


# ------------------------------------------------------------------------------------- c. the Lemire fallback
@pytest.mark.parametrize("n", [3, 5, 8])
def test_lemire_fallback(lib, n):
    """A buffered uint32 planted so that the bounded draw's low word falls below n_empty (0, or ceil(2^32 / n_empty)):
    the draw is then accepted or rejected and redrawn by the threshold rule.  Board and the whole RNG state after the
    step (and after one more) against the NumPy generator holding the same buffered value."""
    kw = SR.BULK_CFGS["log2_all"]
    boards, seeds, actions, plant, stats = SR.lemire_setup(n)
    L = len(boards)
    assert stats["accepted"] >= 20 and stats["rejected"] >= 20             # (test_sized_ref_cpu.py asserts the rest)
    env = _env(n, kw, L, record_merged=True, record_prev_board=True, record_reward64=True)
    envp = _env(n, kw, L, packed_mask=True)
    refs = []
    for i in range(L):
        r = SR.SizedRef(n, kw, saturate=True)
        r.reset(seeds[i])
        r.inject(SR.values(boards[i]))
        refs.append(r)
    for v in (env, envp):
        v.reset(seed=seeds)
        _put_boards(v, boards, n)
    uint = env.rng_uint.cpu().numpy().view(np.uint32).copy()
    state = env.state.cpu().numpy().view(np.uint32).copy()
    for i in np.flatnonzero(plant >= 0):
        uint[i] = plant[i]
        state[i] |= lib.LS_HAS_U32
        s = refs[i].rng_state
        s["has_uint32"], s["uinteger"] = 1, int(plant[i])
        refs[i].rng_state = s
    for v in (env, envp):
        v.rng_uint.copy_(torch.from_numpy(uint.view(np.int32)).to(DEV))
        v.state.copy_(torch.from_numpy(state.view(np.int32)).to(DEV))
    _assert_rng(env, refs, range(L), "planted")
    live = np.ones(L, dtype=bool)
    prev_exp = boards.copy()
    for t in range(2):
        a = torch.from_numpy(actions[t]).to(DEV)
        env.step_into(a)
        envp.step_into(a)
        res = _check_step(lib, n, env, envp, refs, np.flatnonzero(live), actions[t], prev_exp, (n, "lemire", t))
        _assert_rng(env, refs, np.flatnonzero(live), (n, "lemire", t))
        for i, r in res.items():
            prev_exp[i] = SR.exponents(refs[i].board).reshape(-1)
            if r["terminated"] or r["truncated"]:
                live[i] = False


# ------------------------------------------------------------------------- d. auto-reset after termination
@pytest.mark.parametrize("rng", ["pcg64", "philox"])
@pytest.mark.parametrize("n", [3, 6, 8])
def test_auto_reset_after_termination(lib, n, rng):
    """Boards one move from their end, auto_reset on.  A lane that terminates reports the terminal step's reward and
    flags with F_RESET, and everything it holds afterwards is a fresh reset(seed + stride); every other lane is the
    reference's step -- under Philox that pins the spawned cell and value to the rule, not just 'one new tile'."""
    L, stride, seed0 = 257, 1000, 5
    kw = SR.BULK_CFGS["log2_all"]
    fam = [b for name, b in SR.family_boards(n, 11, dense=16)
           if name.startswith(("hole", "pair", "checker")) or name.endswith("t")]
    boards = np.stack([fam[i % len(fam)] for i in range(L)])
    env = _env(n, kw, L, rng=rng, auto_reset=True, reset_stride=stride, record_merged=True, record_prev_board=True,
               record_reward64=True)
    envp = _env(n, kw, L, rng=rng, auto_reset=True, reset_stride=stride, packed_mask=True)
    refs = []
    for i in range(L):
        r = SR.SizedRef(n, kw, saturate=True, rng=rng)
        r.reset(seed0 + i)
        r.inject(SR.values(boards[i]))
        refs.append(r)
    for v in (env, envp):
        v.reset(seed=seed0)
        _put_boards(v, boards, n)
    arng = np.random.default_rng(n)
    n_term = n_live_spawn = 0
    for t in range(4):
        acts = np.zeros(L, dtype=np.uint8)
        for i in range(L):                             # a valid move where there is one (an invalid one now and then)
            ok = [a for a, m in enumerate(refs[i].mask()) if m]
            acts[i] = ok[arng.integers(len(ok))] if ok and arng.random() < 0.9 else arng.integers(4)
        a = torch.from_numpy(acts).to(DEV)
        env.step_into(a)
        envp.step_into(a)
        fl, flp = env.flags.cpu().numpy(), envp.flags.cpu().numpy()
        board = unpack_planes(env.board.cpu().numpy(), n)
        boardp = unpack_planes(envp.board.cpu().numpy(), n)
        prev = unpack_planes(env.prev_board.cpu().numpy(), n)
        r32, r64 = env.reward.cpu().numpy(), env.reward64.cpu().numpy()
        mask, bits = env.mask.cpu().numpy(), envp.mask_bits.cpu().numpy()
        obs, obsp, merged = env.obs.cpu().numpy(), envp.obs.cpu().numpy(), env.merged.cpu().numpy()
        st, sd = env.state.cpu().numpy().view(np.uint32), env.seed.cpu().numpy().view(np.uint64)
        score = env.score.cpu().numpy()
        ended = []
        for i in range(L):
            w = (n, rng, t, i)
            before = SR.exponents(refs[i].board).reshape(-1)
            r = refs[i].step(int(acts[i]))
            end = r["terminated"] or r["truncated"]
            want = (lib.F_CHANGED * r["changed"]) | (lib.F_TERMINATED * r["terminated"]) | \
                (lib.F_TRUNCATED * r["truncated"]) | (lib.F_INVALID * r["invalid"]) | \
                (lib.F_OVERFLOW * r["saturated"]) | (lib.F_RESET * end)
            assert fl[i] == want and flp[i] == want, (w, fl[i], want)
            assert r64[i] == r["reward"] and r32[i] == np.float32(r["reward"]), w       # the terminal step's reward
            assert np.array_equal(merged[i], SR.pad_merged(r["merged"], n)) and np.array_equal(prev[i], before), w
            if end:
                n_term += r["terminated"]
                ended.append(i)
                refs[i].reset(refs[i].seed + stride)                       # a fresh episode of the reference
                assert int(score[i]) == 0, w
            else:
                n_live_spawn += r["changed"]
                assert int(score[i]) == r["score"], w
            e = SR.exponents(refs[i].board).reshape(-1)
            assert np.array_equal(board[i], e) and np.array_equal(boardp[i], e), w
            m = refs[i].mask()
            assert mask[i].tolist() == m and int(bits[i]) == SR.mask_bits(m), w
            assert np.array_equal(obs[i], refs[i].obs()) and np.array_equal(obsp[i], refs[i].obs()), w
            assert int(sd[i]) == refs[i].seed, w
            assert int(st[i] & 0xFFFFF) == refs[i].steps and 1 << int((st[i] >> 20) & 31) == refs[i].max_tile_seen, w
            assert st[i] & lib.LS_ACTIVE, w
        if rng == "pcg64":
            _assert_rng(env, refs, range(L), (n, rng, t))                  # state, inc, uinteger, LS_HAS_U32
        else:
            assert not (st & lib.LS_HAS_U32).any()
    assert n_term >= L // 8 and n_live_spawn >= L // 8, (n_term, n_live_spawn)


# ------------------------------------------------------------------------- e. move / obs / symmetries directly
PAD = 0x5A5A5A5A5A5A5A5A


def _planes(e, n, stride):
    """Planes of the boards e in a [W, stride] buffer whose pad columns hold PAD."""
    L = len(e)
    buf = torch.full((words(n), stride), PAD, dtype=torch.int64, device=DEV)
    buf[:, :L] = torch.from_numpy(pack_planes(e, n)).to(DEV)
    return buf


@pytest.mark.parametrize("n", ALL_SIZES)
def test_move_obs_symmetries_direct(lib, n):
    boards = SR.bulk_setup(n, "log2_all")[0]                               # the family boards: exponents 0..15
    L, W, LEN, s = len(boards), words(n), n * (n // 2), lib.stream_handle(DEV)
    assert boards.max() == 15 and boards.min() == 0
    src = _planes(boards, n, L + 5)
    vals = [SR.values(b).reshape(n, n) for b in boards]
    # ---- move: all four actions of every board (lane i takes action (i + k) % 4 in round k), then action 7
    changed = np.zeros((L, 4), dtype=bool)
    n_over = n_full = 0
    for k in range(5):
        acts = ((np.arange(L) + k) % 4).astype(np.uint8) if k < 4 else np.full(L, 7, dtype=np.uint8)
        out = torch.full((W, L + 9), PAD, dtype=torch.int64, device=DEV)
        mer = torch.full((L + 1, LEN), 0xEE, dtype=torch.uint8, device=DEV)
        flg = torch.full((L + 1,), 0xEE, dtype=torch.uint8, device=DEV)
        acts_d = torch.from_numpy(acts).to(DEV)
        lib.check(lib.lib().g2048_sized_move(n, src.data_ptr(), L + 5, acts_d.data_ptr(), out.data_ptr(), L + 9,
                                             mer.data_ptr(), flg.data_ptr(), L, s))
        got, gm, gf = unpack_planes(out[:, :L].cpu().numpy(), n), mer.cpu().numpy(), flg.cpu().numpy()
        assert (out[:, L:] == PAD).all() and (src[:, L:] == PAD).all()     # the pad columns stay untouched
        assert (gm[L] == 0xEE).all() and gf[L] == 0xEE
        if k == 4:
            assert (gf[:L] == lib.F_BADACTION).all() and np.array_equal(got, boards) and not gm[:L].any()
            continue
        for i in range(L):
            new, merged, ch = SR.move(vals[i], int(acts[i]))
            over = 65536 in merged
            assert np.array_equal(got[i], np.minimum(SR.exponents(new), 15).reshape(-1)), (n, k, i)
            assert np.array_equal(gm[i], SR.pad_merged(merged, n)), (n, k, i)
            assert gf[i] == (lib.F_CHANGED * ch) | (lib.F_OVERFLOW * over), (n, k, i)
            changed[i, acts[i]] = ch
            n_over += over
            n_full += len(merged) == LEN
    assert n_over >= 4 and n_full >= 4
    # ---- obs in the three modes (raw 32768.0, one-hot channel 15) and the int8 mask
    for mode, code, scale in (("raw", 0, 1.0), ("log2", 1, 0.3), ("onehot", 2, 1.0)):
        OW = _ow(n, mode)
        obs = torch.full((L + 1, OW), -7.0, dtype=torch.float32, device=DEV)
        mask = torch.full((L + 1, 4), 9, dtype=torch.int8, device=DEV)
        lib.check(lib.lib().g2048_sized_obs(n, src.data_ptr(), L + 5, code, scale, obs.data_ptr(), mask.data_ptr(), L,
                                            s))
        want = SR.obs_of(SR.values(boards).reshape(L, n, n), mode, scale)
        assert np.array_equal(obs[:L].cpu().numpy(), want) and (obs[L] == -7.0).all()
        assert np.array_equal(mask[:L].cpu().numpy(), changed.astype(np.int8)) and (mask[L] == 9).all()
        if mode == "raw":
            assert want.max() == 32768.0
        if mode == "onehot":
            assert want.reshape(L, n * n, 17)[:, :, 15].any()
    # ---- the 8 symmetries and their action maps, np.rot90 / np.fliplr in get_symmetries order
    acts = (np.arange(L) % 4).astype(np.uint8)
    ob = torch.full((W, 8 * L + 3), PAD, dtype=torch.int64, device=DEV)
    oa = torch.full((8 * L + 1,), 0xEE, dtype=torch.uint8, device=DEV)
    acts_d = torch.from_numpy(acts).to(DEV)
    lib.check(lib.lib().g2048_sized_symmetries(n, src.data_ptr(), L + 5, acts_d.data_ptr(), ob.data_ptr(), 8 * L + 3,
                                               oa.data_ptr(), L, s))
    got = unpack_planes(ob[:, :8 * L].cpu().numpy(), n).reshape(8, L, n * n)
    ga = oa.cpu().numpy()
    assert (ob[:, 8 * L:] == PAD).all() and ga[8 * L] == 0xEE
    for i in range(L):
        for k, (sb, sa, _) in enumerate(SR.symmetries(boards[i].reshape(n, n), int(acts[i]))):
            assert np.array_equal(got[k, i], sb.reshape(-1)) and ga[k * L + i] == sa, (n, k, i)
    torch.cuda.synchronize()
