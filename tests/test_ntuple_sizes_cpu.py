"""CPU: the n-tuple value network at every board size 2..8 and every tuple shape, against an INDEPENDENT reference.

tests/test_ntuple_host.py holds the host build (tests/native/ntuple_host.cpp, compiled from csrc/g2048_ntuple_core.h, the
header the kernels compile) to the recorded fixture, which has sizes 2, 3, 4, 5, 8, tuples of 2..4 cells and feature
counts that are multiples of 8.  Here the host build and the package's Python statement (rl2048_amd.ntuple) are compared
with tests/ntuple_pyref.py, written from include/g2048_ntuple.h alone, on inputs generated from seeds:

* V, Q_0, Q_1 and the choices at every size 2..8 (both games at 4 x 4), on tests/ntuple_ref.board_set: a dead board,
  boards with one valid action, ties, tiles on either side of every word boundary, exponent 15 in every cell of a
  tuple, random fills; NTuplePolicy.q_values / NTupleNetwork.value at sizes 6 and 7;
* the TD(0) update at every size and on two networks with 5- and 6-cell tuples, at (lr_num, lr_shift) = (1, 6) and at
  (65536, 0), where rows clamp on both sides and entries wrap; lengths of 0, T, T + 3 and -1;
* raw feature lists of 1, 3, 5 and 7 features (k = 2..6, two on one offset): the remainder of the loops over features.

Every comparison is ==, and every coverage condition is asserted from the reference's own counts before anything is
compared.  Not a parity claim for the GPU path (that is tests/test_gpu_ntuple_sizes.py).
"""
import numpy as np
import pytest

import ntuple_pyref as PR
import ntuple_ref as NR
from ntuple_ref import ALL_SIZES, INVALID

VALUE_CASES = [(n, False) for n in ALL_SIZES] + [(4, True)]
TD_NETS = list(ALL_SIZES) + list(NR.WIDE_NETS) + [NR.FULL_NET]
LRS = [(1, 6), (65536, 0)]


def check_coverage(c):
    """What the board set is there for, from the reference's answers alone."""
    for q, a in ((c["q0"], c["a0"]), (c["q1"], c["a1"])):
        ok = q != INVALID
        nvalid = ok.sum(axis=1)
        assert (nvalid == 0).sum() >= 1 and (a[nvalid == 0] == 0).all(), "no dead board"
        assert (nvalid == 1).sum() >= 1, "no board with exactly one valid action"
        best = np.where(ok, q, INVALID).max(axis=1)
        assert ((((q == best[:, None]) & ok).sum(axis=1) > 1) & (nvalid >= 2)).sum() >= 1, "no tie"
    assert ((c["q1"] < 0) & (c["q1"] != INVALID)).any(), "no negative Q_1"
    assert (c["ex"] == 15).any() and len(c["ex"]) > 256 and len(c["ex"]) % 64 != 0


# ------------------------------------------------------------------------------------------------------- boards
@pytest.mark.parametrize("size,native4", VALUE_CASES, ids=[f"N{n}-{'core4x4' if k else 'sized'}" for n, k in VALUE_CASES])
def test_host_build_values_and_choices_equal_the_reference(size, native4):
    c = NR.size_case(size)
    check_coverage(c)
    net, planes = c["net"], c["planes"]
    np.testing.assert_array_equal(NR.host_values(net, native4, planes), c["v"])
    a0, q0 = NR.host_choose(net, native4, 0, planes)
    np.testing.assert_array_equal(q0, c["q0"])
    np.testing.assert_array_equal(a0, c["a0"])
    a1, q1 = NR.host_choose(net, native4, 1, planes[:, c["i1"]])
    np.testing.assert_array_equal(q1, c["q1"])
    np.testing.assert_array_equal(a1, c["a1"])


@pytest.mark.parametrize("size", [6, 7])
def test_python_class_equals_the_reference(size):
    from rl2048_amd import NTuplePolicy

    c = NR.size_case(size)
    net = c["net"]
    p0, p1 = NTuplePolicy(net, 0), NTuplePolicy(net, 1)
    for i in range(0, len(c["ex"]), 2):
        e = c["ex"][i]
        assert net.value(e) == int(c["v"][i]), i
        assert p0.q_values(e) == c["q0"][i].tolist() and p0.choose(e) == int(c["a0"][i]), i
    crafted = len(c["i1"]) - {6: 12, 7: 10}[size]
    picked = [k for k in range(len(c["i1"])) if (c["ex"][c["i1"][k]] == 0).sum() <= 6 or k >= crafted + 8]
    assert len(picked) >= 4                       # the emptier boards cost the Python statement up to a second each
    for k in picked:
        e = c["ex"][c["i1"][k]]
        assert p1.q_values(e) == c["q1"][k].tolist() and p1.choose(e) == int(c["a1"][k]), k


# ----------------------------------------------------------------------------------------------------------- TD
def check_td_coverage(want, lr, T, n, lengths):
    new, rows, abs_delta, info = want
    assert rows > 50 and abs_delta > 0 and info["entries"] > 100
    assert {0, T, T + 3, -1} <= set(lengths.tolist())
    if lr == (65536, 0):
        assert info["clamp_hi"] >= 1 and info["clamp_lo"] >= 1 and info["wrapped"] >= 1, info
    else:
        assert info["clamp_hi"] == info["clamp_lo"] == 0, info


@pytest.mark.parametrize("lr", LRS, ids=["lr1-6", "lr65536-0"])
@pytest.mark.parametrize("name", TD_NETS, ids=[f"N{x}" if isinstance(x, int) else x for x in TD_NETS])
def test_host_build_update_equals_the_reference(name, lr):
    c = NR.td_reference(name, *lr)
    net = c["net"]
    T, n = c["actions"].shape
    check_td_coverage(c["want"], lr, T, n, c["lengths"])
    new, rows, abs_delta, info = c["want"]
    for native4 in ((False, True) if net.size == 4 else (False,)):
        got, r, d = NR.host_td(net, native4, c["before"], c["planes"], c["actions"], c["flags"], c["lengths"], *lr)
        assert (r, d) == (rows, abs_delta)
        np.testing.assert_array_equal(got, new)
    assert int((new != c["before"]).sum()) > 100
    # lengths T + 3 and -1 behave as T and 0
    ln = np.clip(c["lengths"], 0, T).astype(np.int32)
    same = PR.td_update(NR.features_of(net), c["before"], net.size, c["ex"], c["actions"], c["flags"], ln, *lr)
    assert same[1:3] == (rows, abs_delta) and np.array_equal(same[0], new)


# ------------------------------------------------------------------------------------------------- raw feature lists
@pytest.mark.parametrize("nf", [1, 3, 5, 7])
@pytest.mark.parametrize("size", [4, 6])
def test_raw_feature_lists(size, nf):
    c = NR.raw_case(size, nf)
    feats, net, planes = c["feats"], c["net"], c["planes"]
    assert len(feats) == nf and nf % 4 != 0
    ks = [len(cells) for _, cells in feats]
    assert ks == [3, 3, 2, 4, 6, 5, 2][:nf] and (nf < 2 or feats[0][0] == feats[1][0])
    np.testing.assert_array_equal(NR.host_values(net, False, planes), c["v"])
    for depth, sel in ((0, np.arange(len(c["ex"]))), (1, c["i1"])):
        for native4 in ((False, True) if size == 4 else (False,)):
            ga, gq = NR.host_choose(net, native4, depth, planes[:, sel])
            np.testing.assert_array_equal(gq, c[f"q{depth}"])
            np.testing.assert_array_equal(ga, c[f"a{depth}"])
    for lr in LRS:
        new, rows, abs_delta, info = c["td"][lr]
        assert rows > 50 and info["entries"] >= nf
        got, r, d = NR.host_td(net, False, c["w"], c["bplanes"], c["actions"], c["flags"], c["lengths"], *lr)
        assert (r, d) == (rows, abs_delta)
        np.testing.assert_array_equal(got, new)
