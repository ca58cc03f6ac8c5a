"""CPU checks of the n-tuple value network (csrc/g2048_ntuple_core.h, include/g2048_ntuple.h, rl2048_amd.NTupleNetwork /
NTuplePolicy), through a TEST-ONLY host build (tests/native/ntuple_host.cpp):

* V, Q_0, Q_1 and the choices of tests/golden/ntuple.npz (recorded by tests/golden/make_golden_ntuple.py from a model
  written out there on its own) on every fixture board, in the sized game and, at N = 4, the 4 x 4 game of
  g2048_core.h; the Python class gives the same (on a subset at depth 1, where a board costs it up to a second);
* dead boards, ties, the floor of a negative chance total, the symmetry expansion;
* the fixture episodes (the real reference's run_episode with that player as action_gen) row for row, in 16-step
  chunks, so the suspend / resume state is exercised too, with the policy stream untouched;
* the TD(0) update: the fixture cases, a truncated last row, an invalid recorded row, the clamp, two features on one
  entry;
* the C ABI on host buffers: every G2048_EINVAL case before any HIP call, zero counts OK; the Python refusals.

Every comparison is ==.  Not a parity claim for the GPU path (that is tests/test_gpu_ntuple.py).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ntuple_ref as NR
import sized_ref as SR
from ntuple_ref import BOARD_SIZES, INVALID
from test_scripted_host import _bare_agent, _Call, _ids, _pcg_state_after

ROOT = NR.ROOT


@pytest.fixture(scope="module")
def gold():
    return NR.golden()


_nets: dict = {}


def net_of(size):
    if size not in _nets:
        _nets[size] = NR.make_net(size)
    return _nets[size]


# ------------------------------------------------------------------------------------------------------- boards
BOARD_CASES = [(n, False) for n in BOARD_SIZES] + [(4, True)]


@pytest.mark.parametrize("size,native4", BOARD_CASES, ids=[f"N{n}-{'core4x4' if k else 'sized'}" for n, k in BOARD_CASES])
def test_host_build_gives_the_fixture_values_and_choices(gold, size, native4):
    net = net_of(size)
    e = gold[f"b{size}_boards"]
    planes = SR.pack_planes(e, size)
    assert len(e) >= 290
    np.testing.assert_array_equal(NR.host_values(net, native4, planes), gold[f"b{size}_v"])
    a0, q0 = NR.host_choose(net, native4, 0, planes)
    np.testing.assert_array_equal(q0, gold[f"b{size}_q0"])
    np.testing.assert_array_equal(a0, gold[f"b{size}_a0"])
    i1 = gold[f"b{size}_i1"]
    a1, q1 = NR.host_choose(net, native4, 1, planes[:, i1])
    np.testing.assert_array_equal(q1, gold[f"b{size}_q1"])
    np.testing.assert_array_equal(a1, gold[f"b{size}_a1"])
    # what the fixture is there for: dead boards (action 0, all INT64_MIN), one valid move, ties to the lowest action
    for q, a in ((q0, a0), (q1, a1)):
        valid = q != INVALID
        nvalid = valid.sum(axis=1)
        assert (nvalid == 0).sum() >= 1 and (a[nvalid == 0] == 0).all()
        best = np.where(valid, q, INVALID).max(axis=1)
        ties = ((q == best[:, None]) & valid).sum(axis=1) > 1
        assert ties.sum() >= (4 if len(q) > 100 else 1)          # the depth-1 subset is 30 boards at N = 8
        first = np.argmax((q == best[:, None]) & valid, axis=1)
        np.testing.assert_array_equal(a[nvalid > 0], first[nvalid > 0])
    assert (q0 < 0).any() and ((q1 < 0) & (q1 != INVALID)).any()             # Q may be negative


@pytest.mark.parametrize("size", BOARD_SIZES)
def test_python_class_gives_the_fixture_values_and_choices(gold, size):
    from rl2048_amd import NTuplePolicy

    net = net_of(size)
    e = gold[f"b{size}_boards"]
    p0, p1 = NTuplePolicy(net, 0), NTuplePolicy(net, depth=1)
    for i in range(0, len(e), 1 if size <= 4 else 3):
        assert net.value(e[i]) == int(gold[f"b{size}_v"][i])
        assert p0.q_values(e[i]) == gold[f"b{size}_q0"][i].tolist() and p0.choose(e[i]) == int(gold[f"b{size}_a0"][i])
    i1 = gold[f"b{size}_i1"]
    step = {2: 1, 3: 2, 4: 6, 5: 6, 8: 6}[size]
    for k in range(0, len(i1), step):
        b = e[i1[k]]
        assert p1.q_values(b) == gold[f"b{size}_q1"][k].tolist(), (size, k)
        vals = np.where(b > 0, np.int64(1) << b.astype(np.int64), 0).reshape(size, size)
        # the reference's signature: (state as Game2048Env.state gives it, action mask or None)
        assert p1(vals.tolist(), None) == int(gold[f"b{size}_a1"][k]) == p1(vals.tolist(), np.ones(4, dtype=np.int8))


def test_dead_boards_ties_and_validation():
    from rl2048_amd import NTupleNetwork, NTuplePolicy

    net = net_of(2)
    p = NTuplePolicy(net)
    assert p.depth == 0 and p.q_values([1, 2, 2, 1]) == [INVALID] * 4 and p.choose([1, 2, 2, 1]) == 0
    a, q = NR.host_choose(net, False, 1, SR.pack_planes(np.array([[1, 2, 2, 1]], dtype=np.uint8), 2))
    assert a.tolist() == [0] and q.tolist() == [[INVALID] * 4]
    # zero weights: every Q_0 is the gain alone, so a board whose moves gain the same ties and takes the lowest action
    zero = NR.make_net(4, seed=False)
    b = np.zeros(16, dtype=np.uint8)
    b[5] = 1
    a, q = NR.host_choose(zero, True, 0, SR.pack_planes(b[None], 4))
    assert q.tolist() == [[0, 0, 0, 0]] and a.tolist() == [0]
    b[0], b[5] = 0, 0
    b[3] = 2                       # top-right corner: up and right are invalid, down ties with left
    a, q = NR.host_choose(zero, False, 0, SR.pack_planes(b[None], 4))
    assert q.tolist() == [[INVALID, INVALID, 0, 0]] and a.tolist() == [2]
    assert NTuplePolicy(zero).choose(b) == 2
    for bad in (dict(depth=2), dict(depth=-1), dict(depth=1.0), dict(depth="1"), dict(depth=True), dict(depth=None)):
        with pytest.raises(ValueError):
            NTuplePolicy(net, **bad)
    with pytest.raises(TypeError):
        NTuplePolicy(object())
    with pytest.raises(ValueError):
        p.q_values([1, 2, 3])
    for bad in ((1,), (0, 0), (0, 4), (-1, 0), (0, 1, 2, 3, 0, 1, 2)):
        with pytest.raises(ValueError):
            NTupleNetwork(2, [bad], device="cpu")
    for bad_size in (1, 9, 4.0, "4"):
        with pytest.raises(ValueError):
            NTupleNetwork(bad_size, device="cpu")
    with pytest.raises(ValueError):
        NTupleNetwork(4, [(0, 1)] * 17, device="cpu")


def test_the_floor_of_a_negative_chance_total():
    """A depth-1 value whose chance total is negative and not divisible by 10 #empty: floor, not C's truncation."""
    from rl2048_amd import NTuplePolicy

    h = NR.host()
    assert h.nt_floor_div(-7, 2) == -4 and h.nt_floor_div(7, 2) == 3 and h.nt_floor_div(-8, 2) == -4
    assert h.nt_floor_div(-1, 150) == -1 and h.nt_floor_div(0, 150) == 0 and -7 // 2 == -4
    # one table of one tuple with large negative weights on "both cells empty" and "a 2 and an empty cell" (they
    # outweigh the next move's gain): the total over the 3 empty cells of the afterstate is -6000459, 30 does not
    # divide it, the floor is -200016 and C's truncation would give -200015
    net = NR.make_net(2, tuples=[(0, 1)], seed=False)
    w = np.zeros(net.n_weights, dtype=np.int32)
    w[0], w[1] = -100001, -7
    net.load_state_dict(dict(net.state_dict(), weights=w))
    pol = NTuplePolicy(net, 1)
    b = np.array([[0, 0, 1, 0]], dtype=np.uint8)
    want = pol.q_values(b[0])
    empties = 3
    found = False
    for a in range(4):
        if want[a] != INVALID and want[a] < 0:
            # recompute the total the slow way to show it is not divisible
            from rl2048_amd.ntuple import move_score
            m, g = move_score(tuple(int(x) for x in b[0]), 2, a)
            tot = sum(wt * max([v for v in pol._q0(m[:c] + (e,) + m[c + 1:]) if v != INVALID], default=0)
                      for c in range(4) if m[c] == 0 for e, wt in ((1, 9), (2, 1)))
            assert tot < 0 and want[a] == tot // (10 * empties)
            found = found or tot % (10 * empties) != 0
    assert found and want == [-200016, -200016, INVALID, INVALID]
    a1, q1 = NR.host_choose(net, False, 1, SR.pack_planes(b, 2))
    assert q1[0].tolist() == want and int(a1[0]) == pol.choose(b[0])


def _sym_images(e, n):
    g = e.reshape(n, n)
    out = []
    for k in range(4):
        r = np.rot90(g, k)
        out += [r, r.T]
    return [x.reshape(-1) for x in out]


@pytest.mark.parametrize("size", BOARD_SIZES)
def test_symmetry_expansion(gold, size):
    from rl2048_amd import NTupleNetwork
    from rl2048_amd.ntuple import dihedral_images

    net = net_of(size)
    assert len(net.features) == 8 * len(net.tuples) == {2: 16, 3: 40, 4: 40, 5: 72, 8: 112}[size]
    assert net.n_weights == sum(16 ** len(t) for t in net.tuples)
    if size == 4:
        assert NTupleNetwork.default_tuples(4) == [(0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 4, 5), (1, 2, 5, 6), (5, 6, 9, 10)]
        assert net.n_weights * 4 == 5 * (1 << 18)                                  # 1.25 MiB
        assert dihedral_images((0, 1), 4) == [(0, 1), (3, 7), (15, 14), (12, 8), (0, 4), (12, 13), (15, 11), (3, 2)]
    if size == 2:
        assert NTupleNetwork.default_tuples(2) == [(0, 1), (0, 1, 2, 3)]
    if size == 8:
        assert net.n_weights * 4 == 14 * (1 << 18)                                 # 3.5 MiB
    # images that coincide stay separate features: the centre square's 8 images are the same 4 cells
    cells = [tuple(sorted(c)) for t, _, c in net.features if t == len(net.tuples) - 1]
    assert len(cells) == 8 and (size not in (3, 4) or len(set(cells)) == (1 if size == 4 else 4))
    e = gold[f"b{size}_boards"][60:90]
    v = NR.host_values(net, False, SR.pack_planes(e, size))
    for i in range(len(e)):
        imgs = np.stack(_sym_images(e[i], size))
        assert len(imgs) == 8
        np.testing.assert_array_equal(NR.host_values(net, False, SR.pack_planes(imgs, size)), np.full(8, v[i]))
        assert net.value(imgs[3]) == int(v[i])


def test_fill_hash_and_state_dict():
    from rl2048_amd import NTupleNetwork
    from rl2048_amd.ntuple import hash_weights

    net = NTupleNetwork(3, device="cpu")
    assert net.weights.dtype.is_floating_point is False and int(net.weights.abs().sum()) == 0
    net.fill_hash(7)
    w = net.host_weights()
    M = (1 << 64) - 1
    for table, index in ((0, 0), (1, 4095), (4, 65535), (2, 12345)):      # the docstring's formula, in Python integers
        x = (7 * 0x9E3779B97F4A7C15 + table * 0xBF58476D1CE4E5B9 + index * 0x94D049BB133111EB + 1) & M
        x ^= x >> 31
        x = (x * 0xD6E8FEB86659FD93) & M
        x ^= x >> 29
        assert int(w[net.offsets[table] + index]) == (x >> 48) - 32768
    assert w.dtype == np.int32 and w.min() < -32000 and w.max() > 32000 and hash_weights(0, 5, 7).tolist() == w[:5].tolist()
    st = net.state_dict()
    assert set(st) == {"size", "tuples", "weights"} and all(isinstance(v, (np.ndarray, np.integer)) for v in st.values())
    other = NTupleNetwork(3, device="cpu")
    other.load_state_dict(st)
    assert np.array_equal(other.host_weights(), w) and other.value([1] * 9) == net.value([1] * 9)
    with pytest.raises(ValueError):
        NTupleNetwork(4, device="cpu").load_state_dict(st)
    with pytest.raises(ValueError):
        other.load_state_dict(dict(st, weights=st["weights"].astype(np.int64)))


# ------------------------------------------------------------------------------------------- reference episodes
EP_CASES = [(c, False) for c in range(7)] + [(c, True) for c in range(2)]


@pytest.mark.parametrize("c,native4", EP_CASES, ids=[f"case{c}-{'core4x4' if k else 'sized'}" for c, k in EP_CASES])
def test_host_build_plays_the_reference_episodes(gold, c, native4):
    case = NR.ep_cases()[c]
    size, depth = case["size"], case["depth"]
    assert size == 4 or not native4
    P = f"e{c}_"
    lens = gold[P + "length"]
    assert len(lens) == 2
    s = 0
    for i, T in enumerate(lens.tolist()):
        es, ps = int(gold[P + "env_seed"][i]), int(gold[P + "policy_seed"][i])
        planes, acts, rews, flags, st = NR.host_play(net_of(size), native4, depth, case["env"], es, ps)
        where = f"case {case['name']} episode {i}"
        assert len(acts) == T, where
        np.testing.assert_array_equal(SR.unpack_planes(planes, size), gold[P + "boards"][s:s + T], err_msg=where)
        np.testing.assert_array_equal(acts, gold[P + "actions"][s:s + T], err_msg=where)
        np.testing.assert_array_equal(rews.view(np.uint64), gold[P + "rewards"][s:s + T].view(np.uint64), err_msg=where)
        assert np.float64(st.total).view(np.uint64) == gold[P + "total_reward"][i].view(np.uint64), where
        assert (1 << st.mt) == int(gold[P + "max_tile"][i]), where
        assert (flags[:-1] & 6 == 0).all() and flags[-1] & 6, where
        assert bool(flags[-1] & 2) == bool(gold[P + "terminated"][i]), where
        assert (flags & 8 == 0).all(), where                       # never an invalid action, also with the mask off
        # the policy stream is never drawn from: it is default_rng(policy_seed)'s initial state
        assert (st.pol.s_lo, st.pol.s_hi, st.pol.has_uint32, st.pol.uinteger) == _pcg_state_after(ps, 0), where
        s += T
    assert s == len(gold[P + "actions"])


def test_fixture_covers_what_the_issue_lists(gold):
    got = [(c["size"], c["depth"], c["env"].get("max_steps"), c["env"].get("use_action_mask", True))
           for c in NR.ep_cases()]
    assert got == [(4, 0, None, True), (4, 1, 60, True), (2, 0, None, True), (3, 0, None, True), (5, 0, 40, True),
                   (8, 0, 48, True), (3, 1, None, False)]
    assert int(gold["frac_bits"]) == 10
    assert not any(k.endswith("weights") for k in gold)            # only seeds are stored


# ----------------------------------------------------------------------------------------------------------- TD
@pytest.mark.parametrize("size,native4", [(3, False), (4, False), (4, True)])
def test_td_fixture_cases(gold, size, native4):
    net = net_of(size)
    planes, actions, flags, lengths = NR.td_case(size)
    lr_num, lr_shift = (int(x) for x in gold[f"td{size}_lr"])
    before = net.host_weights()
    want, rows, abs_delta = NR.td_expected(size, before)
    got, r, d = NR.host_td(net, native4, before, planes, actions, flags, lengths, lr_num, lr_shift)
    assert (r, d) == (rows, abs_delta) and rows > 100
    np.testing.assert_array_equal(got, want)
    assert int((got != before).sum()) == len(gold[f"td{size}_pos"]) > 500
    if size == 4:       # truncated episodes in the case: their last rows are skipped
        assert (~gold["td4_terminated"]).sum() >= 1 and rows == int(lengths.sum()) - int((~gold["td4_terminated"]).sum())


def test_td_truncated_last_row_contributes_nothing():
    net = net_of(3)
    planes, actions, flags, lengths = NR.td_case(3)
    before = net.host_weights()
    full, rows, _ = NR.host_td(net, False, before, planes, actions, flags, lengths, 3, 5)
    fl = flags.copy()
    i = 2
    L = int(lengths[i])
    fl[L - 1, i] = 0x01 | 0x04                                      # truncated instead of terminated
    trunc, rows_t, _ = NR.host_td(net, False, before, planes, actions, fl, lengths, 3, 5)
    assert rows_t == rows - 1
    # the same as the update without that row at all, with the row before it still bootstrapping from it
    only = np.zeros_like(lengths)
    only[i] = L
    a_t, r_a, _ = NR.host_td(net, False, before, planes, actions, fl, only, 3, 5)
    a_f, r_f, _ = NR.host_td(net, False, before, planes, actions, flags, only, 3, 5)
    assert r_a == L - 1 and r_f == L
    last = NR.host_td(net, False, before, planes[:, L - 1:L, i:i + 1], actions[L - 1:L, i:i + 1],
                      flags[L - 1:L, i:i + 1], np.array([1], dtype=np.int32), 3, 5)
    assert last[1] == 1
    np.testing.assert_array_equal((a_f.astype(np.int64) - a_t), (last[0].astype(np.int64) - before))
    np.testing.assert_array_equal(full.astype(np.int64) - trunc, a_f.astype(np.int64) - a_t)


def test_td_invalid_row_clamp_and_double_hit():
    from rl2048_amd.ntuple import FRAC_BITS

    h = NR.host()
    # the clamp and the floor of the shift, against Python integers
    for d, num, sh in ((1 << 46, 65536, 0), (-(1 << 46), 65536, 0), (1 << 46, 65536, 40), (-(1 << 46) - 1, 65535, 40), (-5, 1, 1), (5, 1, 1), (-1, 1, 40), ((1 << 30) + 5, 1, 0),
                       (-(1 << 30) - 5, 1, 0), (12345678, 3, 5), (-12345678, 3, 5)):
        assert h.nt_td_step(d, num, sh) == max(-(1 << 30), min(1 << 30, (d * num) >> sh)), (d, num, sh)
    # one episode of one row on a 2 x 2 board [1, 1, 0, 0]: action 3 (left) merges to [2, 0, 0, 0], gain 4; action 0
    # (up) is invalid: the afterstate is the board itself and the gain 0
    net = NR.make_net(2, tuples=[(0, 1)], seed=False)
    w0 = np.zeros(net.n_weights, dtype=np.int32)
    board = SR.pack_planes(np.array([[1, 1, 0, 0]], dtype=np.uint8), 2).reshape(1, 1, 1)
    one = np.array([1], dtype=np.int32)
    term = np.array([[0x03]], dtype=np.uint8)
    # afterstate [2, 0, 0, 0]: the 8 images of (0, 1) read (2, 0) twice, (0, 2) twice and (0, 0) four times: index 2
    # gets two adds, index 32 two, index 0 four -- features of one board that hit the same entry add twice
    w0[2], w0[32], w0[0] = 100, 200, -50
    v = 2 * 100 + 2 * 200 + 4 * -50
    got, rows, d = NR.host_td(net, False, w0, board, np.array([[3]], dtype=np.uint8), term, one, 1, 0)
    assert rows == 1 and d == abs(0 - v) == 400
    assert (got[2], got[32], got[0]) == (100 - 2 * 400, 200 - 2 * 400, -50 - 4 * 400) and int((got != w0).sum()) == 3
    # invalid recorded row: m = [1, 1, 0, 0]: indices 0x11 twice (rows), 0x01 / 0x10 ... V from the zero entries = 0
    w1 = np.zeros(net.n_weights, dtype=np.int32)
    w1[0x11] = 7
    got, rows, d = NR.host_td(net, False, w1, board, np.array([[0]], dtype=np.uint8), term, one, 1, 0)
    hits = sum(1 for _, _, c in net.features if tuple(int(x) for x in (np.array([1, 1, 0, 0])[list(c)])) == (1, 1))
    assert rows == 1 and d == 7 * hits and got[0x11] == 7 - hits * 7 * hits
    # a two-row episode: row 0's target is (g_1 << F) + V(m_1) with the weights before the call
    ex = np.array([[1, 1, 0, 0], [2, 2, 0, 0]], dtype=np.uint8)
    planes = SR.pack_planes(ex, 2).reshape(1, 2, 1)
    acts = np.array([[3], [3]], dtype=np.uint8)
    fl = np.array([[0x01], [0x03]], dtype=np.uint8)
    got, rows, d = NR.host_td(net, False, w0, planes, acts, fl, np.array([2], dtype=np.int32), 1, 0)
    v0 = v                                           # V([2,0,0,0]) on w0
    v1 = 2 * int(w0[3]) + 2 * int(w0[48]) + 4 * int(w0[0])      # V([3,0,0,0]) = -200
    y0 = (8 << FRAC_BITS) + v1
    assert rows == 2 and d == abs(y0 - v0) + abs(0 - v1)
    # the clamp through the update itself: 2^30 on the entry read four times makes delta -2^32 and the step -2^30; the
    # entries hit twice go to -2^31, and the entry hit four times wraps like np.int32: 2^30 - 4 2^30 = -3 2^30 -> 2^30
    big = np.zeros(net.n_weights, dtype=np.int32)
    big[0] = 1 << 30
    got, rows, d = NR.host_td(net, False, big, board, np.array([[3]], dtype=np.uint8), term, one, 65536, 0)
    assert rows == 1 and d == 1 << 32
    assert int(got[2]) == int(got[32]) == -(1 << 31) and int(got[0]) == 1 << 30 and int((got != big).sum()) == 2


# --------------------------------------------------------------------------------------------------- Python
@pytest.mark.parametrize("method", ["rollout_batch", "evaluate_batch"])
def test_refusals_precede_any_device_call(method):
    from rl2048_amd import NTuplePolicy

    pol = NTuplePolicy(net_of(4))
    play = getattr(_bare_agent(), method)
    with pytest.raises(ValueError, match="pcg64"):
        play([1], [2], rng="philox", action_gen=pol)
    with pytest.raises(ValueError, match="same length"):
        play([1], [2, 3], action_gen=pol)
    if method == "rollout_batch":
        with pytest.raises(ValueError, match="record_probs"):
            play([1], [2], record_probs=True, action_gen=pol)
    with pytest.raises(ValueError, match="board size"):
        getattr(_bare_agent(size=3), method)([1], [2], action_gen=pol)
    with pytest.raises(TypeError, match="run_episode"):
        play([1], [2], action_gen=net_of(4))                       # a network is not a player
    # the mask may be off: the family is chosen without a refusal
    for size, fam in ((4, "ntuple"), (3, "sized_ntuple")):
        a = _bare_agent(size=size, use_action_mask=False)
        assert a._check_scripted(NTuplePolicy(net_of(size), 1), "pcg64", False) == fam
    assert _bare_agent()._paths == {}


def test_agent_refusals_and_tuning_attributes():
    import torch
    from rl2048_amd import ExpectimaxPolicy, NTuplePolicy
    from rl2048_amd.agent import ReinforceAgent

    a = _bare_agent()
    pol = NTuplePolicy(net_of(4))
    with pytest.raises(TypeError, match="NTuplePolicy"):
        a.ntuple_actions(torch.zeros(3, dtype=torch.int64), ExpectimaxPolicy())
    with pytest.raises(ValueError, match="int64"):
        a.ntuple_actions(torch.zeros(3, dtype=torch.int32), pol)
    with pytest.raises(ValueError, match="board size"):
        a.ntuple_actions(torch.zeros(3, dtype=torch.int64), NTuplePolicy(net_of(3)))
    with pytest.raises(TypeError, match="NTupleNetwork"):
        a.ntuple_update(None, pol, 1, 4)
    for lr in ((0, 4), (65537, 4), (1, -1), (1, 41), (1.0, 4), (True, 4)):
        with pytest.raises(ValueError, match="lr_"):
            a.ntuple_update(None, net_of(4), *lr)
    with pytest.raises(TypeError, match="TrajectoryBatch"):
        a.ntuple_update(None, net_of(4), 1, 4)
    with pytest.raises(RuntimeError, match="HIP device"):
        net_of(4).values(torch.zeros(3, dtype=torch.int64))         # no CPU fallback
    v = vars(ReinforceAgent)
    assert v["ntuple_rollout_cap0"] == 512 and v["ntuple_step_budget"] == 2048 and v["ntuple_max_workgroups"] == 0
    assert v["ntuple_rollout_max_rows"] == 1 << 24
    fams = ReinforceAgent._PERSISTENT
    assert fams["ntuple"].ntuple and fams["sized_ntuple"].sized and fams["ntuple"].budget == "ntuple_step_budget"
    assert not fams["search"].ntuple and not fams["ntuple"].search and not fams["ntuple"].scripted


# --------------------------------------------------------------------------------------------------- C ABI
NARGS = {"g2048_ntuple_rollout": 18, "g2048_ntuple_eval": 18, "g2048_sized_ntuple_rollout": 20,
         "g2048_sized_ntuple_eval": 19, "g2048_ntuple_choose": 6, "g2048_sized_ntuple_choose": 7,
         "g2048_ntuple_values": 5, "g2048_sized_ntuple_values": 6, "g2048_ntuple_td_update": 12,
         "g2048_sized_ntuple_td_update": 14}


def test_entry_points_declared_bound_and_exported():
    import rl2048_amd
    from rl2048_amd import _lib

    assert _lib.ABI_VERSION == 17 and {"NTupleNetwork", "NTuplePolicy"} <= set(rl2048_amd.__all__)
    hdr = open(os.path.join(ROOT, "include", "g2048.h")).read()
    assert "#define G2048_ABI_VERSION 17" in hdr and '#include "g2048_ntuple.h"' in hdr
    nh = open(os.path.join(ROOT, "include", "g2048_ntuple.h")).read()
    for name, val in (("FRAC_BITS", 10), ("MAX_DEPTH", 1), ("MIN_CELLS", 2), ("MAX_CELLS", 6), ("MAX_FEATURES", 128),
                      ("MAX_LR_NUM", 65536), ("MAX_LR_SHIFT", 40)):
        assert f"#define G2048_NTUPLE_{name} {val}" in nh and getattr(_lib, "NTUPLE_" + name) == val
    assert _lib.NTUPLE_SYMBOLS == tuple(NARGS)
    for tu in ("g2048_ntuple.hip", "g2048_sized_ntuple.hip"):
        assert any(s.endswith(tu) for s in _lib.SOURCES)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    lib = _lib.lib()
    assert lib.g2048_abi_version() == 17
    for name, nargs in NARGS.items():
        assert f"int {name}(" in nh and f"int {name}(" not in hdr and f" T {name}" in out
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
    assert ctypes.sizeof(_lib.NTupleFeature) == 12 and _lib.NTupleFeature.cells.offset == 5
    assert ctypes.sizeof(_lib.NTuple) == 32 and _lib.NTuple.weights.offset == 16 and _lib.NTuple.n_weights.offset == 24


def _desc(depth=0, size=4, feats=None, n_features=None, weights=True, n_weights=None, features=True):
    """A descriptor on host buffers: (struct, keep-alive).  feats: [(offset, k, cells)] (default: the default net's)."""
    from rl2048_amd import _lib as L

    net = net_of(size)
    if feats is None:
        feats = [(o, len(c), c) for _, o, c in net.features]
    arr = (L.NTupleFeature * max(len(feats), 1))(*[
        L.NTupleFeature(o, k, (ctypes.c_uint8 * 6)(*(list(c) + [0] * 6)[:6]), 0) for o, k, c in feats])
    w = (ctypes.c_int32 * 16)()
    d = L.NTuple(depth, len(feats) if n_features is None else n_features, arr if features else None,
                 ctypes.addressof(w) if weights else None, net.n_weights if n_weights is None else n_weights)
    return d, (arr, w)


def _bad_descriptors(size=4):
    ok = [(0, 4, (0, 1, 2, 3))]
    return {
        "depth2": dict(depth=2), "depth-1": dict(depth=-1), "no-features": dict(features=False),
        "no-weights": dict(weights=False), "n_features0": dict(feats=ok, n_features=0),
        "n_features129": dict(feats=ok * 129), "k1": dict(feats=[(0, 1, (0,))]), "k7": dict(feats=[(0, 7, (0, 1, 2, 3, 4, 5))]),
        "cell-off-board": dict(feats=[(0, 2, (0, size * size))]), "repeated-cell": dict(feats=[(0, 3, (1, 2, 1))]),
        "offset-beyond": dict(feats=[(1, 4, (0, 1, 2, 3))], n_weights=65536),
        "table-beyond": dict(feats=ok, n_weights=65535), "n_weights0": dict(feats=ok, n_weights=0),
    }


class _NtCall(_Call):
    """test_scripted_host._Call (its host buffers and defaults) for the four play entry points: the `script` argument
    holds the descriptor."""

    def __init__(self, L, which):
        super().__init__(L, which)
        self.args["script"], keep = _desc(size=5 if which.startswith("sized") else 4)
        self.keep.append(keep)

    def __call__(self, sus_over=None, out_over=None, **over):
        a = dict(self.args, **over)
        L = self.L
        byref = lambda x: ctypes.byref(x) if x is not None else None
        s = L.Suspend(**dict(self.sus, **(sus_over or {})))
        rows = self.which in ("rollout", "sized_rollout")
        o = (L.Traj(**dict(self.traj, **(out_over or {}))) if rows else L.EvalOut(**dict(self.out, **(out_over or {}))))
        outp = byref(o) if a["traj" if rows else "out"] is not None else None
        head = (byref(a["script"]), byref(a["cfg"]), a["env_state"], a["env_inc"], a["env_buf"], a["pol_state"],
                a["pol_inc"], a["pol_buf"], a["queue"], a["order"], a["n_order"], a["resume"],
                byref(s) if a["sus"] is not None else None, a["n"], a["cap"], outp)
        lib = L.lib()
        if self.which == "rollout":
            return lib.g2048_ntuple_rollout(*head, a["max_workgroups"], a["stream"])
        if self.which == "eval":
            return lib.g2048_ntuple_eval(*head, a["max_workgroups"], a["stream"])
        if self.which == "sized_rollout":
            return lib.g2048_sized_ntuple_rollout(a["size"], *head, a["board_stride"], a["max_workgroups"], a["stream"])
        return lib.g2048_sized_ntuple_eval(a["size"], *head, a["max_workgroups"], a["stream"])


FAMILIES = ("rollout", "eval", "sized_rollout", "sized_eval")


@pytest.fixture(scope="module")
def calls():
    from rl2048_amd import _lib as L

    return {w: _NtCall(L, w) for w in FAMILIES}


@pytest.mark.parametrize("which", FAMILIES)
def test_zero_count_returns_ok_without_a_launch(calls, which):
    call = calls[which]
    assert call(n_order=0) == call.L.G2048_OK
    assert call(n_order=0, order=None, n=0) == call.L.G2048_OK
    size = 5 if which.startswith("sized") else 4
    assert call(n_order=0, script=_desc(depth=1, size=size)[0]) == call.L.G2048_OK
    cfg = call.L.EnvCfg.from_buffer_copy(call.cfg)
    cfg.use_action_mask = 0                                          # the mask may be off
    assert call(cfg=cfg, n_order=0) == call.L.G2048_OK


COMMON = [dict(script=None), dict(cfg=None), dict(env_state=None), dict(env_inc=None), dict(env_buf=None),
          dict(pol_state=None), dict(pol_inc=None), dict(pol_buf=None), dict(queue=None), dict(sus=None), dict(n=-1),
          dict(n=1 << 31), dict(n_order=-1), dict(n_order=5), dict(order=None, n_order=3), dict(order=None, resume=1),
          dict(cap=0), dict(cap=-1), dict(cap=1 << 31), dict(max_workgroups=-1)]
CASES = {"rollout": COMMON + [dict(traj=None), dict(n=1 << 30, n_order=4, cap=1 << 11)],
         "eval": COMMON + [dict(out=None)],
         "sized_rollout": COMMON + [dict(traj=None), dict(board_stride=31), dict(size=1), dict(size=9), dict(size=0)],
         "sized_eval": COMMON + [dict(out=None), dict(size=1), dict(size=9)]}
EINVAL_CASES = [(w, c) for w in FAMILIES for c in CASES[w]]


@pytest.mark.parametrize("which,over", EINVAL_CASES, ids=[f"{w}-{_ids(c)}" for w, c in EINVAL_CASES])
def test_einval_before_any_launch(calls, which, over):
    L = calls[which].L
    assert calls[which](**over) == L.G2048_EINVAL
    assert L.lib().g2048_last_error()


@pytest.mark.parametrize("which", FAMILIES)
def test_bad_descriptors_cfg_probs_and_null_members_are_einval(calls, which):
    call = calls[which]
    L = call.L
    size = 5 if which.startswith("sized") else 4
    for name, kw in _bad_descriptors(size).items():
        d, keep = _desc(size=size, **kw)
        assert call(script=d) == L.G2048_EINVAL, name
    # a cell that is on a 5 x 5 board and not on a 4 x 4 one
    d, keep = _desc(size=size, feats=[(0, 2, (0, 20))])
    assert call(script=d, n_order=0) == (L.G2048_OK if size == 5 else L.G2048_EINVAL)
    cfg = L.EnvCfg.from_buffer_copy(call.cfg)
    cfg.reward_mode = 5
    assert call(cfg=cfg) == L.G2048_EINVAL
    for field in ("board", "meta", "total", "list", "count"):
        assert call(sus_over={field: None}) == L.G2048_EINVAL, field
    for field in ("lengths", "totals", "max_tile", "final_board"):
        assert call(out_over={field: None}) == L.G2048_EINVAL, field
    if which in ("rollout", "sized_rollout"):
        assert call(out_over={"probs": call._buf(ctypes.c_float, 4 * 8 * call.n)}) == L.G2048_EINVAL
        assert b"probs" in L.lib().g2048_last_error()
        for field in ("boards", "actions", "rewards", "flags"):
            assert call(out_over={field: None}) == L.G2048_EINVAL, field


def test_choose_values_and_update_einval_and_zero_counts():
    from rl2048_amd import _lib as L

    lib = L.lib()
    bufs = [(ctypes.c_uint64 * 64)() for _ in range(8)]
    b, a, q, fl, ln, sc, stt, act = (ctypes.addressof(x) for x in bufs)
    ok, keep = _desc()
    ok5, keep5 = _desc(size=5)
    r = ctypes.byref
    assert lib.g2048_ntuple_choose(r(ok), b, 0, a, q, None) == L.G2048_OK
    assert lib.g2048_ntuple_choose(r(ok), b, 0, a, None, None) == L.G2048_OK
    assert lib.g2048_sized_ntuple_choose(5, r(ok5), b, 0, a, q, None) == L.G2048_OK
    assert lib.g2048_ntuple_values(r(ok), b, 0, q, None) == L.G2048_OK
    assert lib.g2048_sized_ntuple_values(5, r(ok5), b, 0, q, None) == L.G2048_OK
    td = lambda d=ok, n=2, T=4, num=3, sh=5, **kw: lib.g2048_ntuple_td_update(
        r(d) if d is not None else None, kw.get("boards", b), kw.get("actions", act), kw.get("flags", fl),
        kw.get("lengths", ln), n, T, num, sh, kw.get("scratch", sc), kw.get("stats", stt), None)
    tds = lambda size=5, d=ok5, n=2, T=4, num=3, sh=5, stride=8, **kw: lib.g2048_sized_ntuple_td_update(
        size, r(d) if d is not None else None, kw.get("boards", b), stride, kw.get("actions", act), kw.get("flags", fl),
        kw.get("lengths", ln), n, T, num, sh, kw.get("scratch", sc), kw.get("stats", stt), None)
    assert td(n=0) == td(T=0) == tds(n=0) == tds(T=0, stride=0) == L.G2048_OK
    for name, kw in _bad_descriptors().items():
        d, k = _desc(**kw)
        d5, k5 = _desc(size=5, **(kw if name != "cell-off-board" else dict(feats=[(0, 2, (0, 25))])))
        assert lib.g2048_ntuple_choose(r(d), b, 4, a, q, None) == L.G2048_EINVAL, name
        assert lib.g2048_sized_ntuple_choose(5, r(d5), b, 4, a, q, None) == L.G2048_EINVAL, name
        assert lib.g2048_ntuple_values(r(d), b, 4, q, None) == L.G2048_EINVAL, name
        assert lib.g2048_sized_ntuple_values(5, r(d5), b, 4, q, None) == L.G2048_EINVAL, name
        assert td(d=d) == L.G2048_EINVAL and tds(d=d5) == L.G2048_EINVAL, name
        assert lib.g2048_last_error()
    for args in ((None, b, 4, a), (r(ok), None, 4, a), (r(ok), b, 4, None), (r(ok), b, -1, a), (r(ok), b, 1 << 31, a)):
        assert lib.g2048_ntuple_choose(*args, q, None) == L.G2048_EINVAL
        assert lib.g2048_ntuple_values(*args[:3], q if args[3] is not None else None, None) == L.G2048_EINVAL
    for size in (0, 1, 9):
        assert lib.g2048_sized_ntuple_choose(size, r(ok), b, 4, a, q, None) == L.G2048_EINVAL
        assert lib.g2048_sized_ntuple_values(size, r(ok), b, 4, q, None) == L.G2048_EINVAL
        assert tds(size=size) == L.G2048_EINVAL
    for bad in (dict(d=None), dict(num=0), dict(num=65537), dict(sh=-1), dict(sh=41), dict(n=-1), dict(T=-1),
                dict(n=1 << 31), dict(T=1 << 31), dict(n=1 << 21, T=1 << 20), dict(boards=None), dict(actions=None),
                dict(flags=None), dict(lengths=None), dict(scratch=None), dict(stats=None)):
        assert td(**bad) == L.G2048_EINVAL, bad
        assert tds(**dict(bad, **({"stride": bad.get("n", 2) * bad.get("T", 4)} if "n" in bad or "T" in bad else {}))) \
            == L.G2048_EINVAL, bad
    assert tds(stride=7) == L.G2048_EINVAL and b"board_stride" in lib.g2048_last_error()
