"""CPU checks of the expectimax player (csrc/g2048_search_core.h, include/g2048_search.h, rl2048_amd.ExpectimaxPolicy),
through a TEST-ONLY host build (tests/native/search_host.cpp):

* the host build and ExpectimaxPolicy both give the Q values and choices of tests/golden/search.npz (recorded by
  tests/golden/make_golden_search.py from a player written out there on its own) on every fixture board -- random
  fills, full boards, boards with one valid move, dead boards, symmetric boards that tie -- at every recorded depth,
  in the 4 x 4 game of g2048_core.h and in the sized game.  The host build is run on all of them; the Python class on
  every board at depth 0 and, for N <= 4, depth 1, on every fifth (N = 5) / tenth (N = 8) at depth 1 and on a few at
  depth 2, where a board costs it up to a second;
* the host build plays every fixture episode (the real reference's run_episode with that player as action_gen) row for
  row, in chunks, so the suspend / resume state is exercised too, and leaves the policy stream untouched;
* a non-default weight set changes choices;
* ExpectimaxPolicy validation, the refusals of rollout_batch / evaluate_batch / search_actions;
* the C ABI: declared in g2048_search.h and not in g2048.h, exported, bound, ABI 17, sizeof(g2048_search) == 20, every
  G2048_EINVAL case on host buffers before any launch, zero counts OK.

Not a parity claim for the GPU path (that is tests/test_gpu_search.py); it localises logic bugs on the CPU.
"""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import sized_ref as SR
from test_scripted_host import ScState, _bare_agent, _Call, _ids, _pcg_state_after
from test_sized_host import EpCfg, ep_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "rl-2048-with-reinforce-and-actor-critic_amd", "csrc")
DEFAULT_W = (4, 16, 1, 2)
BOARD_SIZES = (2, 3, 4, 5, 8)


def _sources():
    return [os.path.join(NATIVE, "search_host.cpp")] + [os.path.join(CSRC, h) for h in (
        "g2048_search_core.h", "g2048_scripted_core.h", "g2048_sized_core.h", "g2048_core.h")]


@functools.lru_cache(maxsize=None)
def search_host():
    """The host build, compiled on first use (tests/test_gpu_search.py holds the kernels to it too)."""
    so = os.path.join(NATIVE, "libsearch_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in _sources()):
        tmp = f"{so}.{os.getpid()}.tmp"   # build aside, then rename: parallel workers never load a partial file
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-o", tmp, _sources()[0]],
                       check=True)
        os.replace(tmp, so)
    L = ctypes.CDLL(so)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    choose = [ctypes.c_int, u32p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    L.sr_choose4.argtypes = choose
    L.sr_choose_sized.argtypes = [ctypes.c_int] + choose
    play = [ctypes.c_int, u32p, ctypes.POINTER(EpCfg), ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64,
            ctypes.POINTER(ScState), ctypes.c_int64] + [ctypes.c_void_p] * 4
    L.sr_play4.restype = ctypes.c_int64
    L.sr_play4.argtypes = play
    L.sr_play_sized.restype = ctypes.c_int64
    L.sr_play_sized.argtypes = [ctypes.c_int] + play
    return L


@pytest.fixture(scope="module")
def sh():
    return search_host()


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "search.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def gold():
    return golden()


def _w(weights):
    return (ctypes.c_uint32 * 4)(*weights)


def native_choose(size, native4, depth, planes, weights=DEFAULT_W):
    """The host build's choice on [W, m] planes (int64 / uint64): (actions uint8 [m], q int64 [m, 4]).  native4: the
    4 x 4 game of g2048_core.h (size must be 4); else the sized game."""
    sh = search_host()
    planes = np.ascontiguousarray(planes).view(np.uint64).reshape(SR.words(size), -1)
    m = planes.shape[1]
    acts = np.full(m, 255, dtype=np.uint8)
    q = np.full((m, 4), -7, dtype=np.int64)
    args = (depth, _w(weights), planes.ctypes.data, m, acts.ctypes.data, q.ctypes.data)
    assert (sh.sr_choose4(*args) if native4 else sh.sr_choose_sized(size, *args)) == 0
    return acts, q


def fixture_boards(gold, size, depth):
    """(exponents [m, N*N], q [m, 4], choice [m]) of the fixture at this size and depth."""
    e = gold[f"b{size}_boards"]
    if depth == 2:
        e = e[gold[f"b{size}_i2"]]
    return e, gold[f"b{size}_q{depth}"], gold[f"b{size}_a{depth}"]


BOARD_CASES = [(n, d, False) for n in BOARD_SIZES for d in (0, 1)] + [(n, 2, False) for n in (2, 3, 4)] + \
              [(4, d, True) for d in (0, 1, 2)]


@pytest.mark.parametrize("size,depth,native4", BOARD_CASES,
                         ids=[f"N{n}-d{d}-{'core4x4' if k else 'sized'}" for n, d, k in BOARD_CASES])
def test_host_build_gives_the_fixture_q_values_and_choices(gold, size, depth, native4):
    e, q, a = fixture_boards(gold, size, depth)
    assert len(e) >= (40 if depth == 2 else 290) and tuple(gold["weights"]) == DEFAULT_W
    acts, got = native_choose(size, native4, depth, SR.pack_planes(e, size))
    np.testing.assert_array_equal(got, q)
    np.testing.assert_array_equal(acts, a)
    # what the fixture is there for
    nvalid = (q >= 0).sum(axis=1)
    ties = ((q == q.max(axis=1, keepdims=True)) & (q >= 0)).sum(axis=1) > 1
    full = (e != 0).all(axis=1)
    assert (nvalid == 0).sum() >= 2 and (nvalid == 1).sum() >= 2 and ties.sum() >= 4 and full.sum() >= 5
    assert (a[nvalid == 0] == 0).all() and (q[np.arange(len(a)), a][nvalid > 0] == q.max(axis=1)[nvalid > 0]).all()


@pytest.mark.parametrize("size", BOARD_SIZES)
def test_expectimax_policy_gives_the_fixture_q_values_and_choices(gold, size):
    from rl2048_amd import ExpectimaxPolicy

    checked = 0
    for depth in (0, 1, 2) if size <= 4 else (0, 1):
        e, q, a = fixture_boards(gold, size, depth)
        pol = ExpectimaxPolicy(depth=depth)
        step = (10 if size == 8 else 5) if (size > 4 and depth == 1) else (4, 4, 4, 4, 14)[size] if depth == 2 else 1
        for i in range(0, len(e), step):
            assert pol.q_values(e[i]) == q[i].tolist(), (size, depth, i)
            vals = np.where(e[i] > 0, np.int64(1) << e[i].astype(np.int64), 0).reshape(size, size)
            # the reference's signature: (state as Game2048Env.state gives it, action mask or None)
            assert pol(vals.tolist(), None) == int(a[i]) == pol(vals.tolist(), np.ones(4, dtype=np.int8))
            checked += 1
    assert checked >= 290 + 29


def test_a_non_default_weight_set_changes_choices(gold):
    from rl2048_amd import ExpectimaxPolicy

    e = gold["b4_boards"]
    planes = SR.pack_planes(e, 4)
    a_def, _ = native_choose(4, True, 0, planes)
    a_emp, q_emp = native_choose(4, True, 0, planes, (0, 1, 0, 0))
    a_emp_s, q_emp_s = native_choose(4, False, 0, planes, (0, 1, 0, 0))
    np.testing.assert_array_equal(a_emp, a_emp_s)
    np.testing.assert_array_equal(q_emp, q_emp_s)
    assert int((a_def != a_emp).sum()) > 0
    pol = ExpectimaxPolicy(depth=0, w_merge=0, w_empty=1, w_smooth=0, w_corner=0)
    for i in range(0, len(e), 3):
        assert pol.q_values(e[i]) == q_emp[i].tolist() and pol.choose(e[i]) == int(a_emp[i])
    # (0, 1, 0, 0): Q is the afterstate's empty count
    assert int(q_emp.max()) <= 15
    # the largest weights at N = 8, depth 1, where the values are largest (Python integers are the yardstick)
    big = ExpectimaxPolicy(depth=1, w_merge=4096, w_empty=4096, w_smooth=4096, w_corner=4096)
    idx = np.arange(60, 64)
    _, q_big = native_choose(8, False, 1, SR.pack_planes(gold["b8_boards"][idx], 8), (4096,) * 4)
    for k, i in enumerate(idx):
        assert big.q_values(gold["b8_boards"][i]) == q_big[k].tolist()


# ------------------------------------------------------------------------------------------- reference episodes
def play(sh, size, native4, depth, env_kw, env_seed, pol_seed, weights=DEFAULT_W, chunk=16, most=1 << 16):
    """test_scripted_host.play for the search player."""
    W = SR.words(size)
    cfg = ep_cfg(env_kw)
    st = ScState()
    boards, acts, rews, flags = [], [], [], []
    fresh = 1
    while True:
        b = np.zeros((chunk, W), dtype=np.uint64)
        a = np.zeros(chunk, dtype=np.uint8)
        r = np.zeros(chunk, dtype=np.float64)
        f = np.zeros(chunk, dtype=np.uint8)
        args = (depth, _w(weights), ctypes.byref(cfg), fresh, env_seed, pol_seed, ctypes.byref(st), chunk,
                b.ctypes.data, a.ctypes.data, r.ctypes.data, f.ctypes.data)
        k = sh.sr_play4(*args) if native4 else sh.sr_play_sized(size, *args)
        assert 1 <= k <= chunk
        boards.append(b[:k]); acts.append(a[:k]); rews.append(r[:k]); flags.append(f[:k])
        fresh = 0
        if st.ended:
            break
        assert k == chunk and st.t < most
    out = (np.concatenate(boards).T.copy(), np.concatenate(acts), np.concatenate(rews), np.concatenate(flags), st)
    assert st.t == st.sc == len(out[1])
    return out


def ep_cases():
    return json.loads(str(golden()["ep_cases"]))


# (fixture case, game): the 4 x 4 cases run in both games
EP_CASES = [(c, False) for c in range(8)] + [(c, True) for c in range(2)]


@pytest.mark.parametrize("c,native4", EP_CASES, ids=[f"case{c}-{'core4x4' if k else 'sized'}" for c, k in EP_CASES])
def test_host_build_plays_the_reference_episodes(sh, gold, c, native4):
    case = ep_cases()[c]
    size, depth = case["size"], case["depth"]
    assert size == 4 or not native4
    P = f"e{c}_"
    lens = gold[P + "length"]
    assert len(lens) == 2
    s = 0
    for i, T in enumerate(lens.tolist()):
        es, ps = int(gold[P + "env_seed"][i]), int(gold[P + "policy_seed"][i])
        planes, acts, rews, flags, st = play(sh, size, native4, depth, case["env"], es, ps)
        where = f"case {case['name']} episode {i}"
        assert len(acts) == T, where
        np.testing.assert_array_equal(SR.unpack_planes(planes, size), gold[P + "boards"][s:s + T], err_msg=where)
        np.testing.assert_array_equal(acts, gold[P + "actions"][s:s + T], err_msg=where)
        np.testing.assert_array_equal(rews.view(np.uint64), gold[P + "rewards"][s:s + T].view(np.uint64), err_msg=where)
        assert np.float64(st.total).view(np.uint64) == gold[P + "total_reward"][i].view(np.uint64), where
        assert (1 << st.mt) == int(gold[P + "max_tile"][i]), where
        assert (flags[:-1] & 6 == 0).all() and flags[-1] & 6, where
        assert (flags & 8 == 0).all(), where                       # never an invalid action, also with the mask off
        # the policy stream is never drawn from: it is default_rng(policy_seed)'s initial state
        assert (st.pol.s_lo, st.pol.s_hi, st.pol.has_uint32, st.pol.uinteger) == _pcg_state_after(ps, 0), where
        s += T
    assert s == len(gold[P + "actions"])


def test_fixture_covers_what_the_issue_lists(gold):
    cases = ep_cases()
    got = [(c["size"], c["depth"], c["env"].get("max_steps"), c["env"].get("use_action_mask", True)) for c in cases]
    assert got == [(4, 0, None, True), (4, 1, 60, True), (3, 1, None, True), (3, 2, None, True), (2, 2, None, True),
                   (5, 1, 40, True), (8, 0, 48, True), (3, 1, None, False)]
    assert "reward_mode" not in cases[0]["env"] and cases[1]["env"]["bonus_mode"] == "raw"
    for n in BOARD_SIZES:
        assert int(gold[f"b{n}_boards"].max()) == 14


# --------------------------------------------------------------------------------------------------- Python
def test_expectimax_policy_validation():
    from rl2048_amd import ExpectimaxPolicy, _lib

    p = ExpectimaxPolicy()
    assert (p.depth, p.w_merge, p.w_empty, p.w_smooth, p.w_corner) == (1, 4, 16, 1, 2)
    p = ExpectimaxPolicy(np.int64(2), 0, 4096, np.uint8(7), 1)
    s = p._search()
    assert isinstance(s, _lib.Search) and (s.depth, s.w_merge, s.w_empty, s.w_smooth, s.w_corner) == (2, 0, 4096, 7, 1)
    assert "depth=2" in repr(p) and callable(p)
    for bad in (dict(depth=3), dict(depth=-1), dict(depth=1.0), dict(depth="1"), dict(depth=None), dict(depth=True),
                dict(w_merge=4097), dict(w_empty=-1), dict(w_smooth=1.5), dict(w_corner="2"), dict(w_corner=1 << 40)):
        with pytest.raises(ValueError):
            ExpectimaxPolicy(**bad)
    with pytest.raises(ValueError):
        p.q_values([1, 2, 3])                       # not a square board
    assert p.choose([1, 2, 2, 1]) == 0 and p.q_values([1, 2, 2, 1]) == [-1, -1, -1, -1]   # a dead board


@pytest.mark.parametrize("method", ["rollout_batch", "evaluate_batch"])
def test_refusals_precede_any_device_call(method):
    from rl2048_amd import ExpectimaxPolicy

    play = getattr(_bare_agent(), method)
    with pytest.raises(ValueError, match="pcg64"):
        play([1], [2], rng="philox", action_gen=ExpectimaxPolicy())
    with pytest.raises(ValueError, match="same length"):
        play([1], [2, 3], action_gen=ExpectimaxPolicy())
    if method == "rollout_batch":
        with pytest.raises(ValueError, match="record_probs"):
            play([1], [2], record_probs=True, action_gen=ExpectimaxPolicy())
    # the mask may be off: the family is chosen without a refusal
    for size, fam in ((4, "search"), (3, "sized_search")):
        a = _bare_agent(size=size, use_action_mask=False)
        assert a._check_scripted(ExpectimaxPolicy(), "pcg64", False) == fam
    assert _bare_agent()._paths == {}


def test_search_actions_refusals_and_tuning_attributes():
    import torch
    from rl2048_amd import ExpectimaxPolicy, PriorityPolicy
    from rl2048_amd.agent import ReinforceAgent

    a = _bare_agent()
    with pytest.raises(TypeError, match="ExpectimaxPolicy"):
        a.search_actions(torch.zeros(3, dtype=torch.int64), PriorityPolicy(PriorityPolicy.URDL))
    with pytest.raises(ValueError, match="int64"):
        a.search_actions(torch.zeros(3, dtype=torch.int32), ExpectimaxPolicy())
    v = vars(ReinforceAgent)
    assert v["search_rollout_cap0"] == 256 and v["search_step_budget"] == 256 and v["search_max_workgroups"] == 0
    assert v["search_rollout_max_rows"] == 1 << 24 and v["eval_step_budget"] == 4096
    fams = ReinforceAgent._PERSISTENT
    assert fams["search"].search and fams["sized_search"].sized and fams["search"].budget == "search_step_budget"
    assert fams["scripted"].budget == fams["deep"].budget == "eval_step_budget" and not fams["scripted"].search


# --------------------------------------------------------------------------------------------------- C ABI
NARGS = {"g2048_search_rollout": 18, "g2048_search_eval": 18, "g2048_sized_search_rollout": 20,
         "g2048_sized_search_eval": 19, "g2048_search_choose": 6, "g2048_sized_search_choose": 7}


def test_entry_points_declared_bound_and_exported():
    from rl2048_amd import _lib

    assert _lib.ABI_VERSION == 17
    hdr = open(os.path.join(ROOT, "include", "g2048.h")).read()
    assert "#define G2048_ABI_VERSION 17" in hdr and '#include "g2048_search.h"' in hdr
    sr = open(os.path.join(ROOT, "include", "g2048_search.h")).read()
    assert "typedef struct g2048_search" in sr and "#define G2048_SEARCH_MAX_DEPTH 2" in sr
    assert f"#define G2048_SEARCH_MAX_WEIGHT {_lib.SEARCH_MAX_WEIGHT}" in sr and _lib.SEARCH_MAX_WEIGHT == 4096
    assert _lib.SEARCH_SYMBOLS == tuple(NARGS)
    assert _lib.SCRIPTED_SYMBOLS == ("g2048_scripted_rollout", "g2048_scripted_eval", "g2048_sized_scripted_rollout",
                                     "g2048_sized_scripted_eval")
    for tu in ("g2048_search.hip", "g2048_sized_search.hip"):
        assert any(s.endswith(tu) for s in _lib.SOURCES)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    lib = _lib.lib()
    assert lib.g2048_abi_version() == 17
    for name, nargs in NARGS.items():
        assert f"int {name}(" in sr and f"int {name}(" not in hdr and f" T {name}" in out
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
    assert ctypes.sizeof(_lib.Search) == 20 and _lib.Search.w_merge.offset == 4 and _lib.Search.w_corner.offset == 16


class _SearchCall(_Call):
    """test_scripted_host._Call (its host buffers and defaults) for the four search entry points: the `script`
    argument holds the search player."""

    def __init__(self, L, which):
        super().__init__(L, which)
        self.args["script"] = L.Search(1, 4, 16, 1, 2)

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
            return lib.g2048_search_rollout(*head, a["max_workgroups"], a["stream"])
        if self.which == "eval":
            return lib.g2048_search_eval(*head, a["max_workgroups"], a["stream"])
        if self.which == "sized_rollout":
            return lib.g2048_sized_search_rollout(a["size"], *head, a["board_stride"], a["max_workgroups"], a["stream"])
        return lib.g2048_sized_search_eval(a["size"], *head, a["max_workgroups"], a["stream"])


FAMILIES = ("rollout", "eval", "sized_rollout", "sized_eval")


@pytest.fixture(scope="module")
def calls():
    from rl2048_amd import _lib as L

    return {w: _SearchCall(L, w) for w in FAMILIES}


def _search(depth=1, w=(4, 16, 1, 2)):
    from rl2048_amd import _lib as L

    return L.Search(depth, *w)


@pytest.mark.parametrize("which", FAMILIES)
def test_zero_count_returns_ok_without_a_launch(calls, which):
    call = calls[which]
    assert call(n_order=0) == call.L.G2048_OK
    assert call(n_order=0, order=None, n=0) == call.L.G2048_OK
    for d in (0, 1, 2):
        assert call(n_order=0, script=_search(d, (4096, 0, 4096, 0))) == call.L.G2048_OK


def test_the_mask_may_be_off(calls):
    for which in FAMILIES:
        call = calls[which]
        cfg = call.L.EnvCfg.from_buffer_copy(call.cfg)
        cfg.use_action_mask = 0
        assert call(cfg=cfg, n_order=0) == call.L.G2048_OK


COMMON = [dict(script=None), dict(script=_search(3)), dict(script=_search(-1)), dict(script=_search(1, (4097, 16, 1, 2))),
          dict(script=_search(0, (4, 4097, 1, 2))), dict(script=_search(2, (4, 16, 1 << 31, 2))),
          dict(script=_search(1, (4, 16, 1, 0xFFFFFFFF))), dict(cfg=None),
          dict(env_state=None), dict(env_inc=None), dict(env_buf=None), dict(pol_state=None), dict(pol_inc=None),
          dict(pol_buf=None), dict(queue=None), dict(sus=None), dict(n=-1), dict(n=1 << 31), dict(n_order=-1),
          dict(n_order=5), dict(order=None, n_order=3), dict(order=None, resume=1), dict(cap=0), dict(cap=-1),
          dict(cap=1 << 31), dict(max_workgroups=-1)]
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
def test_bad_cfg_probs_and_null_members_are_einval(calls, which):
    call = calls[which]
    L = call.L
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


def test_choose_einval_and_zero_count():
    from rl2048_amd import _lib as L

    lib = L.lib()
    boards = (ctypes.c_uint64 * 8)()
    acts = (ctypes.c_uint8 * 8)()
    q = (ctypes.c_int64 * 32)()
    b, a, qq = (ctypes.addressof(x) for x in (boards, acts, q))
    ok = _search()
    assert lib.g2048_search_choose(ctypes.byref(ok), b, 0, a, qq, None) == L.G2048_OK
    assert lib.g2048_search_choose(ctypes.byref(ok), b, 0, a, None, None) == L.G2048_OK
    assert lib.g2048_sized_search_choose(5, ctypes.byref(ok), b, 0, a, qq, None) == L.G2048_OK
    bad = [(None, b, 4, a), (ctypes.byref(_search(3)), b, 4, a), (ctypes.byref(_search(-1)), b, 4, a),
           (ctypes.byref(_search(1, (4, 16, 1, 4097))), b, 4, a), (ctypes.byref(ok), None, 4, a),
           (ctypes.byref(ok), b, 4, None), (ctypes.byref(ok), b, -1, a), (ctypes.byref(ok), b, 1 << 31, a)]
    for sp, bb, n, aa in bad:
        assert lib.g2048_search_choose(sp, bb, n, aa, qq, None) == L.G2048_EINVAL
        assert lib.g2048_sized_search_choose(3, sp, bb, n, aa, qq, None) == L.G2048_EINVAL
        assert lib.g2048_last_error()
    for size in (0, 1, 9):
        assert lib.g2048_sized_search_choose(size, ctypes.byref(ok), b, 4, a, qq, None) == L.G2048_EINVAL
