"""tests/sized_ref.py -- the plain NumPy game / env the late-game GPU tests compare against -- pinned to the REAL
reference, bit for bit, on every recorded state: the whole of tests/golden/sized.npz (episodes from reset, line tables,
crafted boards, symmetry records), tests/golden/symmetries.npz at N = 4, and tests/golden/sized_late.npz (episodes
from injected late-game boards, tests/golden/make_golden_sized_late.py).

The coverage that keeps tests/test_gpu_sized_late.py from being vacuous is asserted here, on the committed fixture and
on the family builder alone: no GPU is needed to know that the GPU tests reach termination, the one-empty-cell spawn,
14+14 and saturated merges, a full merged list, max_tile_seen >= 2^15 and every word-straddling row at every size.
"""
import ctypes
import json
import os

import numpy as np
import pytest

import sized_ref as SR
from test_sized_host import ep_cfg, pack, sh, unpack  # noqa: F401  (sh: the host build of g2048_sized_core.h)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [2, 3, 5, 6, 7, 8]
ALL_SIZES = [2, 3, 4, 5, 6, 7, 8]


def _load(name):
    with np.load(os.path.join(ROOT, "tests", "golden", name)) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def gold():
    return _load("sized.npz")


@pytest.fixture(scope="module")
def late():
    return _load("sized_late.npz")


def _replay(ref, g, p, n, e, start, ln, with_obs):
    """Step ref through fixture steps [start, start + ln) of prefix p and compare every recorded field."""
    for j in range(start, start + ln):
        r = ref.step(int(g[p + "action"][j]))
        where = (p, e, j - start)
        assert np.array_equal(SR.exponents(ref.board).reshape(-1), g[p + "board"][j]), where
        assert np.float64(r["reward"]).view(np.uint64) == g[p + "reward"][j].view(np.uint64), where   # fp64 bits
        assert isinstance(r["reward"], float)
        assert r["terminated"] == bool(g[p + "terminated"][j]) and r["truncated"] == bool(g[p + "truncated"][j]), where
        assert r["invalid"] == bool(g[p + "invalid"][j]), where
        assert r["score"] == int(g[p + "score"][j]) and r["step_index"] == int(g[p + "step_index"][j]), where
        assert np.array_equal(SR.pad_merged(r["merged"], n), g[p + "merged"][j]), where
        assert SR.mask_bits(ref.mask()) == int(g[p + "mask"][j]), where
        assert r["max_tile_seen"] == int(g[p + "max_tile_seen"][j]), where
        if with_obs:
            assert np.array_equal(ref.obs(), g[p + "obs"][j]), where


@pytest.mark.parametrize("n", SIZES)
def test_replays_reset_episodes(gold, n):
    for c, kw in json.loads(str(gold["env_cfgs"])).items():
        p = f"n{n}_c{c}_"
        for e, (seed, start, ln) in enumerate(zip(gold[p + "ep_seed"], gold[p + "ep_start"], gold[p + "ep_len"])):
            ref = SR.SizedRef(n, kw)
            ref.reset(int(seed))
            assert np.array_equal(SR.exponents(ref.board).reshape(-1), gold[p + "reset_board"][e])
            assert np.array_equal(ref.obs(), gold[p + "reset_obs"][e])
            assert SR.mask_bits(ref.mask()) == int(gold[p + "reset_mask"][e])
            _replay(ref, gold, p, n, e, int(start), int(ln), True)


@pytest.mark.parametrize("n", ALL_SIZES)
def test_line_tables(gold, n):
    for a, b, m in zip(gold[f"n{n}_line_in"], gold[f"n{n}_line_out"], gold[f"n{n}_line_merged"]):
        out, merged = SR.slide_row(SR.values(a).tolist())
        assert np.array_equal(SR.exponents(out), b), a
        assert [int(v).bit_length() - 1 for v in merged] == [int(x) for x in m if x], a


@pytest.mark.parametrize("n", SIZES)
def test_crafted_boards_mask_and_done(gold, n):
    for e, m, d in zip(gold[f"n{n}_craft_board"], gold[f"n{n}_craft_mask"], gold[f"n{n}_craft_done"]):
        b = SR.values(e).reshape(n, n)
        assert SR.mask_bits(SR.action_mask(b)) == int(m) and SR.is_done(b) == bool(d), e.reshape(n, n)


@pytest.mark.parametrize("n", [3, 5])
def test_symmetry_records(gold, n):
    for k, (mode, scale) in enumerate(json.loads(str(gold["sym_kinds"]))):
        p = f"n{n}_s{k}_"
        for e, a, obs_out, mask_out, act_out in zip(gold[p + "board_in"], gold[p + "action_in"], gold[p + "obs_out"],
                                                    gold[p + "mask_out"], gold[p + "action_out"]):
            board = SR.values(e).reshape(n, n)
            obs = SR.obs_of(board, mode, scale).reshape((n, n, 17) if mode == "onehot" else (n, n))
            syms = SR.symmetries(obs, int(a), np.array(SR.action_mask(board), dtype=np.int8))
            assert len(syms) == 8
            for s, (sb, sa, sm) in enumerate(syms):
                assert np.array_equal(sb.reshape(-1), obs_out[s]) and sa == int(act_out[s])
                assert np.array_equal(sm, mask_out[s])
            # the images of the board itself carry the images' own masks (what g2048_sized_obs computes from them)
            for (sb, _, _), (_, _, sm) in zip(SR.symmetries(board, int(a)), syms):
                assert SR.action_mask(sb) == [int(x) for x in sm]


def test_symmetry_records_at_size_4():
    z = _load("symmetries.npz")
    for k in range(4):
        p = f"k{k}_"
        for b, m, a, bo, mo, ao in zip(z[p + "board_in"], z[p + "mask_in"], z[p + "action_in"], z[p + "board_out"],
                                       z[p + "mask_out"], z[p + "action_out"]):
            syms = SR.symmetries(b.reshape((4, 4, 17) if b.size == 272 else (4, 4)), int(a), m)
            for s, (sb, sa, sm) in enumerate(syms):
                assert np.array_equal(sb.reshape(-1), bo[s]) and sa == int(ao[s]) and np.array_equal(sm, mo[s])


# ------------------------------------------------------------------------------------------------ the late fixture
@pytest.mark.parametrize("n", ALL_SIZES)
def test_replays_late_episodes(late, n):
    """Every late episode from its injected board: reset(seed), overwrite the board, step.  The boards the fixture
    was made from are the family builder's."""
    fam = SR.family_boards(n, 2048)
    assert [name for name, _ in fam] == [str(s) for s in late[f"n{n}_fam"]]
    for c, kw in json.loads(str(late["env_cfgs"])).items():
        p = f"n{n}_c{c}_"
        assert np.array_equal(np.stack([b for _, b in fam]), late[p + "ep_board"])
        for e, (seed, start, ln) in enumerate(zip(late[p + "ep_seed"], late[p + "ep_start"], late[p + "ep_len"])):
            ref = SR.SizedRef(n, kw)
            ref.reset(int(seed))
            ref.inject(SR.values(late[p + "ep_board"][e]))
            _replay(ref, late, p, n, e, int(start), int(ln), False)
            last = int(start + ln) - 1
            assert bool(late[p + "ep_sat"][e]) == bool((late[p + "merged"][last] == 16).any())
            assert not (late[p + "merged"][int(start):last] == 16).any()       # a saturated merge ends the episode
            assert (late[p + "board"][int(start):last] <= 15).all()
            assert ln == 24 or late[p + "ep_sat"][e] or late[p + "terminated"][last] or late[p + "truncated"][last]


@pytest.mark.parametrize("n", ALL_SIZES)
def test_saturate_mode_differs_only_where_documented(late, n):
    """saturate=True (the kernels' board contract) against the fixture's saturating steps: the board is the
    reference's clipped to 2^15; merged list, score, max_tile_seen, changed and invalid are the reference's; done,
    mask, truncation and the endgame term of the reward may differ only when a clipped tile has a 2^15 neighbour
    (the reference's 65536 cannot merge with it, the nibble board's 2^15 can)."""
    seen = 0
    for c, kw in json.loads(str(late["env_cfgs"])).items():
        p = f"n{n}_c{c}_"
        for e in np.flatnonzero(late[p + "ep_sat"]):
            start, ln = int(late[p + "ep_start"][e]), int(late[p + "ep_len"][e])
            ref = SR.SizedRef(n, kw, saturate=True)
            ref.reset(int(late[p + "ep_seed"][e]))
            ref.inject(SR.values(late[p + "ep_board"][e]))
            _replay(ref, late, p, n, e, start, ln - 1, False)
            j = start + ln - 1
            r = ref.step(int(late[p + "action"][j]))
            gb = late[p + "board"][j].reshape(n, n)
            assert r["saturated"] and np.array_equal(SR.exponents(ref.board), np.minimum(gb, 15))
            assert np.array_equal(SR.pad_merged(r["merged"], n), late[p + "merged"][j])
            assert r["score"] == int(late[p + "score"][j]) and r["max_tile_seen"] == 65536
            assert r["invalid"] == bool(late[p + "invalid"][j]) and r["changed"]
            touch = ((gb[:, :-1] + gb[:, 1:] == 31).any() or (gb[:-1] + gb[1:] == 31).any())   # a 16 beside a 15
            if not touch:
                assert r["terminated"] == bool(late[p + "terminated"][j])
                assert r["truncated"] == bool(late[p + "truncated"][j])
                assert r["reward"] == late[p + "reward"][j]
                assert SR.mask_bits(ref.mask()) == int(late[p + "mask"][j])
            seen += 1
    assert seen > 0


@pytest.mark.parametrize("n", ALL_SIZES)
def test_late_fixture_coverage(late, n):
    cov = SR.late_coverage(late, n)
    for k in ("terminated", "single_empty_spawn", "merge_14_14", "saturated", "full_list", "max_tile_2p15"):
        assert cov[k] >= 1, (n, k, cov)
    # N = 2: one word and a 2-slot list -- no straddling row; everything else is required of it too
    assert sorted(cov["straddle_rows"]) == {2: [], 3: [], 4: [], 5: [3], 6: [2, 5], 7: [2, 4, 6], 8: []}[n]
    assert all(v >= 1 for v in cov["straddle_rows"].values()), cov
    assert SR.late_coverage_ok(cov, n)
    if n >= 3:      # the dense family terminates within its 24 steps under the generator's valid-move policy
        fam = [str(s) for s in late[f"n{n}_fam"]]
        ended = 0
        for c in (int(x) for x in late["env_sel"]):
            p = f"n{n}_c{c}_"
            for e, name in enumerate(fam):
                last = int(late[p + "ep_start"][e] + late[p + "ep_len"][e]) - 1
                ended += name.startswith("dense") and bool(late[p + "terminated"][last])
        assert ended >= 1, n


@pytest.mark.parametrize("n", ALL_SIZES)
def test_family_builder(n):
    fam = SR.family_boards(n, 2048)
    names = [name for name, _ in fam]
    by = {name: b.reshape(n, n) for name, b in fam}
    assert all(b.dtype == np.uint8 and b.shape == (n * n,) and b.max() <= 15 for _, b in fam)
    # lines: every line in every straddling row (cells of two words) and one column
    for r in SR.straddle_rows(n):
        assert (r * n) >> 4 != (r * n + n - 1) >> 4
        for k in range(len(SR.LINES)):
            ln = SR._line(k, n)
            row = by[f"line{k}_r{r}"][r]
            assert np.array_equal(row, ln) or np.array_equal(row, ln[::-1])
    assert any(name.startswith("line") and "_c" in name for name in names)
    assert {2: [], 3: [], 4: [], 5: [3], 6: [2, 5], 7: [2, 4, 6], 8: []}[n] == SR.straddle_rows(n)
    # one empty cell at the first and last nibble of every word, in a board with no merge
    holes = sorted({0, n * n - 1} | {k for k in (15, 16, 31, 32, 47, 48) if k < n * n})
    for k in holes:
        b = by[f"hole{k}"].reshape(-1)
        assert b[k] == 0 and (np.delete(b, k) != 0).all()
        full = b.copy()
        full[k] = 7
        assert SR.is_done(SR.values(full).reshape(n, n))
    # terminal and near-terminal
    assert SR.is_done(SR.values(by["checker12"])) and SR.is_done(SR.values(by["checker14"]))
    assert SR.action_mask(SR.values(by["pair_row"])) == [0, 1, 0, 1]        # left / right only
    assert SR.action_mask(SR.values(by["pair_col"])) == [1, 0, 1, 0]        # up / down only
    # the merged list fills to N * (N // 2)
    for name, acts in (("all1", range(4)), ("all14", range(4)), ("all15", range(4)), ("eq_rows", (1, 3)),
                       ("eq_cols", (0, 2))):
        for a in acts:
            assert len(SR.move(SR.values(by[name]), a)[1]) == n * (n // 2), (name, a)
    # dense: 0..3 empty cells, most tiles 2^8 and above
    dense = [b for name, b in fam if name.startswith("dense")]
    assert sorted({int((b == 0).sum()) for b in dense}) == [0, 1, 2, 3]
    assert np.mean(np.concatenate(dense) >= 8) > 0.5


@pytest.mark.parametrize("cfg_name", sorted(SR.BULK_CFGS))
@pytest.mark.parametrize("n", SIZES)
def test_bulk_differential_keeps_its_lanes(n, cfg_name):
    """The bulk differential of tests/test_gpu_sized_late.py drops a lane after its saturated merge: with the same
    seeds, at most a quarter of the lanes saturate, and its special lanes do what they are there for."""
    refs, boards, seeds, actions, maxt, stepc = SR.bulk_refs(n, cfg_name)
    live = np.ones(len(refs), dtype=bool)
    n_sat = n_trunc = n_term = n_invalid = 0
    for t in range(SR.BULK_STEPS):
        for i in np.flatnonzero(live):
            r = refs[i].step(int(actions[t, i]))
            n_sat += r["saturated"]
            n_trunc += r["truncated"]
            n_term += r["terminated"]
            n_invalid += r["invalid"]
            if r["saturated"] or r["terminated"] or r["truncated"]:
                live[i] = False
    assert n_sat <= SR.BULK_LANES // 4, (n, n_sat)
    assert n_sat >= 1 and n_term >= 1 and n_invalid >= 1, (n_sat, n_term, n_invalid)
    assert (n_trunc >= SR.BULK_LANES // 6) == (SR.BULK_CFGS[cfg_name]["max_steps"] is not None), n_trunc
    assert (maxt > 0).sum() >= SR.BULK_LANES // 3 and (stepc >= 0).sum() >= SR.BULK_LANES // 3


@pytest.mark.parametrize("n", [3, 5, 8])
def test_lemire_setup_reaches_both_outcomes(n):
    """The planted values of the GPU Lemire test enter the fallback; both outcomes occur, over many empty counts (up
    to 63 at N = 8); and the NumPy generator itself, given a planted value, takes it as its next uint32."""
    boards, seeds, actions, plant, stats = SR.lemire_setup(n)
    assert stats["accepted"] >= 20 and stats["rejected"] >= 20, stats
    assert len(stats["sizes"]) >= min(6, n * n - 3) and max(stats["sizes"]) >= (n * n * 3) // 4, stats
    i = int(np.flatnonzero(plant > 0)[0])
    ref = SR.SizedRef(n, SR.BULK_CFGS["log2_all"])
    ref.reset(seeds[i])
    s = ref.rng_state
    s["has_uint32"], s["uinteger"] = 1, int(plant[i])
    ref.rng_state = s
    assert ref.rng_state == s
    assert int(ref.gen.integers(0, 1 << 32, dtype=np.uint32)) == int(plant[i]) and ref.rng_state["has_uint32"] == 0


@pytest.mark.parametrize("n", ALL_SIZES)
def test_late_episodes_through_the_host_build(sh, late, n):  # noqa: F811
    """A localiser: the late fixture through csrc/g2048_sized_core.h compiled for the host (sh_episode_from).  If the
    GPU replay fails and this passes, the fault is in the device compile or the kernel wrapper, not the header's
    logic.  Expectations as in the GPU test: boards clipped to 2^15, the saturating step by saturate=True."""
    W, LEN = SR.words(n), n * (n // 2)
    for c, kw in json.loads(str(late["env_cfgs"])).items():
        p = f"n{n}_c{c}_"
        cfg = ep_cfg(kw)
        for e, (seed, start, ln) in enumerate(zip(late[p + "ep_seed"], late[p + "ep_start"], late[p + "ep_len"])):
            ln, start = int(ln), int(start)
            sl = slice(start, start + ln)
            acts = np.ascontiguousarray(late[p + "action"][sl])
            boards = np.zeros((ln + 1, W), dtype=np.uint64)
            lists = np.zeros((ln, LEN), dtype=np.uint8)
            rewards = np.zeros(ln, dtype=np.float64)
            flags, sadd, masks, mt = (np.zeros(ln, dtype=np.uint32) for _ in range(4))
            rmask = ctypes.c_uint32()
            sh.sh_episode_from(n, int(seed), pack(late[p + "ep_board"][e], n), acts.ctypes.data, ln, ctypes.byref(cfg),
                               boards.ctypes.data, lists.ctypes.data, rewards.ctypes.data, flags.ctypes.data,
                               sadd.ctypes.data, masks.ctypes.data, mt.ctypes.data, ctypes.byref(rmask))
            want = {k: late[p + k][sl].copy() for k in ("reward", "terminated", "truncated", "mask")}
            if late[p + "ep_sat"][e]:
                ref = SR.SizedRef(n, kw, saturate=True)
                ref.reset(int(seed))
                ref.inject(SR.values(late[p + "ep_board"][e]))
                for a in acts:
                    r = ref.step(int(a))
                want["reward"][-1], want["terminated"][-1], want["truncated"][-1] = \
                    r["reward"], r["terminated"], r["truncated"]
                want["mask"][-1] = SR.mask_bits(ref.mask())
            where = (n, c, e)
            assert np.array_equal(unpack(boards[0], n), late[p + "ep_board"][e]), where
            got = np.array([unpack(b, n) for b in boards[1:]])
            assert np.array_equal(got, np.minimum(late[p + "board"][sl], 15)), where
            assert np.array_equal(lists, late[p + "merged"][sl]), where
            assert np.array_equal(rewards.view(np.uint64), want["reward"].view(np.uint64)), where
            assert np.array_equal((flags & 2) != 0, want["terminated"]), where
            assert np.array_equal((flags & 4) != 0, want["truncated"]), where
            assert np.array_equal((flags & 8) != 0, late[p + "invalid"][sl]), where
            assert np.array_equal((flags & 16) != 0, (late[p + "merged"][sl] == 16).any(axis=1)), where
            assert np.array_equal(np.cumsum(sadd.astype(np.int64)), late[p + "score"][sl]), where
            assert np.array_equal(masks, want["mask"]), where
            assert np.array_equal(np.int64(1) << mt.astype(np.int64), late[p + "max_tile_seen"][sl]), where
