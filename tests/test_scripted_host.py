"""CPU checks of scripted play (csrc/g2048_scripted_core.h, include/g2048_scripted.h, rl2048_amd.PriorityPolicy /
UniformPolicy), through a TEST-ONLY host build (tests/native/scripted_host.cpp):

* the host build plays every episode of tests/golden/scripted.npz (recorded from the real reference's
  run_episode(action_gen=action_gen_1 / _2) by tests/golden/make_golden_scripted.py) row for row, in chunks, so the
  suspend / resume state is exercised too, and leaves the policy stream untouched;
* UNIFORM episodes of the host build replay in the CPU oracles (tests/rollout_replay.py) and every action equals
  rollout_replay.choice4 on p = fp32(1) / fp32(k) from the oracle's masks and the draws of default_rng(policy_seed);
* the C ABI: declared, exported, bound, ABI 17, every G2048_EINVAL case before any HIP call, n_order == 0 is OK;
* the Python side: PriorityPolicy validation and choices, the refusals of rollout_batch / evaluate_batch.

Not a parity claim for the GPU path (that is tests/test_gpu_scripted.py); it localises logic bugs on the CPU.
"""
import ctypes
import json
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import rollout_replay as RR
import sized_ref as SR
from test_sized_host import EpCfg, ep_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "rl-2048-with-reinforce-and-actor-critic_amd", "csrc")
PRIORITY, UNIFORM = 0, 1
URDL, URLD = (0, 1, 2, 3), (0, 1, 3, 2)


class ScStream(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint64) for k in ("s_lo", "s_hi", "i_lo", "i_hi")] + \
               [("has_uint32", ctypes.c_uint32), ("uinteger", ctypes.c_uint32)]


class ScState(ctypes.Structure):
    _fields_ = [("board", ctypes.c_uint64 * 4), ("t", ctypes.c_uint32), ("sc", ctypes.c_uint32),
                ("mt", ctypes.c_uint32), ("ended", ctypes.c_uint32), ("total", ctypes.c_double), ("env", ScStream),
                ("pol", ScStream)]


def _sources():
    return [os.path.join(NATIVE, "scripted_host.cpp"), os.path.join(CSRC, "g2048_scripted_core.h"),
            os.path.join(CSRC, "g2048_sized_core.h"), os.path.join(CSRC, "g2048_core.h")]


@pytest.fixture(scope="module")
def sh():
    so = os.path.join(NATIVE, "libscripted_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in _sources()):
        tmp = f"{so}.{os.getpid()}.tmp"   # build aside, then rename: parallel workers never load a partial file
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-o", tmp, _sources()[0]],
                       check=True)
        os.replace(tmp, so)
    L = ctypes.CDLL(so)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    play = [ctypes.c_int, u8p, ctypes.POINTER(EpCfg), ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64,
            ctypes.POINTER(ScState), ctypes.c_int64] + [ctypes.c_void_p] * 4
    L.sc_play4.restype = ctypes.c_int64
    L.sc_play4.argtypes = play
    L.sc_play_sized.restype = ctypes.c_int64
    L.sc_play_sized.argtypes = [ctypes.c_int] + play
    L.sc_order_ok.argtypes = [u8p]
    L.sc_priority_choice.restype = ctypes.c_uint32
    L.sc_priority_choice.argtypes = [u8p, ctypes.c_uint32]
    L.sc_uniform_choice.restype = ctypes.c_uint32
    L.sc_uniform_choice.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_double, ctypes.POINTER(ctypes.c_float)]
    L.sc_seed.argtypes = [ctypes.c_uint64, ctypes.POINTER(ScStream)]
    return L


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(ROOT, "tests", "golden", "scripted.npz")) as z:
        return {k: z[k] for k in z.files}


def _order(o):
    return (ctypes.c_uint8 * 4)(*o)


def _stream_tuple(s):
    return (s.s_lo, s.s_hi, s.i_lo, s.i_hi, s.has_uint32, s.uinteger)


def play(sh, size, native4, kind, order, env_kw, env_seed, pol_seed, chunk=16, most=1 << 20):
    """One episode through the host build, `chunk` steps per call (the state carried the way the kernels' suspend
    protocol carries it).  native4: the 4 x 4 game of g2048_core.h (size must be 4); else the sized game.  Returns
    planes [W, T] uint64, actions, rewards, flags and the final ScState."""
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
        args = (kind, _order(order), ctypes.byref(cfg), fresh, env_seed, pol_seed, ctypes.byref(st), chunk,
                b.ctypes.data, a.ctypes.data, r.ctypes.data, f.ctypes.data)
        k = sh.sc_play4(*args) if native4 else sh.sc_play_sized(size, *args)
        assert 1 <= k <= chunk
        boards.append(b[:k]); acts.append(a[:k]); rews.append(r[:k]); flags.append(f[:k])
        fresh = 0
        if st.ended:
            break
        assert k == chunk and st.t < most
    out = (np.concatenate(boards).T.copy(), np.concatenate(acts), np.concatenate(rews), np.concatenate(flags), st)
    assert st.t == st.sc == len(out[1])
    return out


# ------------------------------------------------------------------------------------------- reference episodes
# (fixture case, game): cases 0..2 are 4 x 4 and run in both games -- g2048_core.h's and the sized one at N = 4
EP_CASES = [(c, False) for c in range(6)] + [(c, True) for c in range(3)]


@pytest.mark.parametrize("c,native4", EP_CASES, ids=[f"case{c}-{'core4x4' if k else 'sized'}" for c, k in EP_CASES])
def test_host_build_plays_the_reference_episodes(sh, gold, c, native4):
    case = json.loads(str(gold["ep_cases"]))[c]
    size = case["size"]
    assert size == 4 or not native4
    P = f"e{c}_"
    lens = gold[P + "length"]
    assert len(lens) == 8 and sorted(set(gold[P + "gen"].tolist())) == [1, 2]
    s = 0
    for i, T in enumerate(lens.tolist()):
        order = URDL if gold[P + "gen"][i] == 1 else URLD
        es, ps = int(gold[P + "env_seed"][i]), int(gold[P + "policy_seed"][i])
        planes, acts, rews, flags, st = play(sh, size, native4, PRIORITY, order, case["env"], es, ps)
        where = f"case {case['name']} episode {i}"
        assert len(acts) == T, where
        np.testing.assert_array_equal(SR.unpack_planes(planes, size), gold[P + "boards"][s:s + T], err_msg=where)
        np.testing.assert_array_equal(acts, gold[P + "actions"][s:s + T], err_msg=where)
        np.testing.assert_array_equal(rews.view(np.uint64), gold[P + "rewards"][s:s + T].view(np.uint64), err_msg=where)
        assert np.float64(st.total).view(np.uint64) == gold[P + "total_reward"][i].view(np.uint64), where
        assert (1 << st.mt) == int(gold[P + "max_tile"][i]), where
        assert (flags[:-1] & 6 == 0).all() and flags[-1] & 6, where
        # PRIORITY never draws: the policy stream is default_rng(policy_seed)'s initial state
        fresh = ScStream()
        sh.sc_seed(ps, ctypes.byref(fresh))
        assert _stream_tuple(st.pol) == _stream_tuple(fresh), where
        s += T
    assert s == len(gold[P + "actions"])


def test_priority_choice_is_the_reference_generators(sh, gold):
    from rl2048_amd import PriorityPolicy

    for order, key in ((URDL, "gen1_choice"), (URLD, "gen2_choice")):
        pol = PriorityPolicy(order)
        for m in range(1, 16):
            mask = np.array([(m >> a) & 1 for a in range(4)], dtype=np.int8)
            want = int(gold[key][m - 1])
            assert pol(None, mask) == want and sh.sc_priority_choice(_order(order), m) == want, (order, m)
    assert PriorityPolicy.URDL == URDL and PriorityPolicy.URLD == URLD
    for order in ((3, 2, 1, 0), (2, 0, 3, 1)):
        for m in range(1, 16):
            want = next(a for a in order if (m >> a) & 1)
            assert sh.sc_priority_choice(_order(order), m) == want
    assert sh.sc_order_ok(_order(URLD)) == 1
    for bad in ((0, 1, 2, 2), (0, 1, 2, 4), (1, 1, 1, 1), (0, 0, 3, 2)):
        assert sh.sc_order_ok(_order(bad)) == 0


# ------------------------------------------------------------------------------------------------- UNIFORM
def _pcg_state_after(seed, draws):
    g = np.random.default_rng(seed)
    if draws:
        g.random(draws)
    s = g.bit_generator.state
    return (s["state"]["state"] & (2 ** 64 - 1), s["state"]["state"] >> 64, s["has_uint32"], s["uinteger"])


UNIFORM_CASES = [(4, True, "R-raw-mask", None, 64), (4, False, "R-raw-mask", None, 64),
                 (4, True, "R-log2-nomask", 200, 64), (4, False, "S-raw-nomask", 200, 64),
                 (3, False, "R-raw-mask", None, 16), (3, False, "R-log2-nomask", 120, 16)]


@pytest.mark.parametrize("size,native4,cfg_name,max_steps,n", UNIFORM_CASES,
                         ids=[f"N{s}-{'core' if c else 'sized'}-{k}" for s, c, k, _, _ in UNIFORM_CASES])
def test_uniform_episodes_replay_and_choose_like_numpy(sh, size, native4, cfg_name, max_steps, n):
    env_kw = dict(RR.CONFIGS[cfg_name], max_steps=max_steps)
    rng = np.random.default_rng(77 + size + n)
    es = rng.integers(0, 2 ** 62, n).astype(np.uint64)
    ps = rng.integers(0, 2 ** 62, n).astype(np.uint64)
    eps = [play(sh, size, native4, UNIFORM, URDL, env_kw, int(e), int(p)) for e, p in zip(es, ps)]
    lens = np.array([len(e[1]) for e in eps], dtype=np.int64)
    T, W = int(lens.max()), SR.words(size)
    planes = np.zeros((W, T, n), dtype=np.uint64)
    acts = np.zeros((T, n), dtype=np.uint8)
    rews = np.zeros((T, n), dtype=np.float64)
    flags = np.zeros((T, n), dtype=np.uint8)
    for i, (b, a, r, f, st) in enumerate(eps):
        planes[:, :lens[i], i], acts[:lens[i], i], rews[:lens[i], i], flags[:lens[i], i] = b, a, r, f
        # one Generator.random() per step, also with one valid action: the stream sits `length` draws in
        assert (st.pol.s_lo, st.pol.s_hi, st.pol.has_uint32, st.pol.uinteger) == _pcg_state_after(int(ps[i]), int(lens[i]))
    final = np.array([[st.board[w] for (_, _, _, _, st) in eps] for w in range(W)], dtype=np.uint64)
    batch = SimpleNamespace(boards=planes if size != 4 else planes[0], actions=acts, rewards=rews, flags=flags,
                            lengths=lens, total_reward=np.array([e[4].total for e in eps]),
                            max_tile=np.array([1 << e[4].mt for e in eps], dtype=np.int64),
                            final_boards=final if size != 4 else final[0], probs=None)
    c = RR.replay_4x4(batch, env_kw, es) if size == 4 else RR.replay_sized(batch, size, env_kw, es)
    masks = c["masks"]
    mb = np.full((T, n), 15, dtype=np.uint8) if masks is None else masks
    k = np.array([bin(m).count("1") for m in range(16)], dtype=np.float32)[mb]
    valid = np.arange(T)[:, None] < lens[None, :]
    assert (k[valid] >= 1).all()
    p = np.where(((mb[:, :, None] >> np.arange(4)) & 1) != 0, (np.float32(1) / np.maximum(k, 1))[:, :, None],
                 np.float32(0)).astype(np.float32)
    assert RR.check_choices(p, acts, lens, ps, False, masks) == int(lens.sum())
    # the host build's own probabilities are these
    got = (ctypes.c_float * 4)()
    for m in range(1, 16):
        sh.sc_uniform_choice(m, 1, 0.5, got)
        assert list(got) == [float(np.float32(1) / np.float32(bin(m).count("1"))) if (m >> a) & 1 else 0.0 for a in range(4)]
    sh.sc_uniform_choice(3, 0, 0.5, got)
    assert list(got) == [0.25] * 4
    if masks is not None:
        assert int((k[valid] == 1).sum()) > 0, "no row with a single valid action: the test proves less than it says"
        assert c["invalid"] == 0
    else:
        assert c["invalid"] > 0
    assert c["terminated"] + c["truncated"] == n and c["bonus"] > 0


# --------------------------------------------------------------------------------------------------- C ABI
NARGS = {"g2048_scripted_rollout": 18, "g2048_scripted_eval": 18, "g2048_sized_scripted_rollout": 20,
         "g2048_sized_scripted_eval": 19}


def test_entry_points_declared_bound_and_exported():
    from rl2048_amd import _lib

    assert _lib.ABI_VERSION == 17
    hdr = open(os.path.join(ROOT, "include", "g2048.h")).read()
    assert "#define G2048_ABI_VERSION 17" in hdr and '#include "g2048_scripted.h"' in hdr
    sc = open(os.path.join(ROOT, "include", "g2048_scripted.h")).read()
    assert "typedef struct g2048_script" in sc and "#define G2048_SCRIPT_PRIORITY 0" in sc
    assert "#define G2048_SCRIPT_UNIFORM 1" in sc and f"#define G2048_SCRIPT_BLOCK {_lib.SCRIPT_BLOCK}" in sc
    assert _lib.SCRIPTED_SYMBOLS == tuple(NARGS)
    for tu in ("g2048_scripted.hip", "g2048_sized_scripted.hip"):
        assert any(s.endswith(tu) for s in _lib.SOURCES)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    lib = _lib.lib()
    assert lib.g2048_abi_version() == 17
    for name, nargs in NARGS.items():
        assert f"int {name}(" in sc and f"int {name}(" not in hdr and f" T {name}" in out
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
    assert ctypes.sizeof(_lib.Script) == 8 and _lib.Script.order.offset == 4


class _Call:
    """One of the four entry points on small host buffers: valid arguments by default, one replaced per case."""

    def __init__(self, L, which):
        self.L, self.which = L, which
        self.n = 4
        self.keep = []
        u64 = lambda k: self._buf(ctypes.c_uint64, k)
        self.cfg = L.EnvCfg(obs_mode=L.OBS_LOG2, reward_mode=1, bonus_mode=0, use_action_mask=1, obs_log2_scale=0.125,
                            base_reward_scale=1.0, invalid_action_penalty=-1.0, max_steps=8)
        self.sus = dict(board=u64(4 * self.n), meta=self._buf(ctypes.c_uint32, 3 * self.n),
                        total=self._buf(ctypes.c_double, self.n), list=self._buf(ctypes.c_int32, self.n),
                        count=self._buf(ctypes.c_uint32, 1))
        self.out = dict(lengths=self._buf(ctypes.c_int32, self.n), totals=self._buf(ctypes.c_double, self.n),
                        max_tile=self._buf(ctypes.c_uint8, self.n), final_board=u64(4 * self.n))
        self.traj = dict(boards=u64(4 * 8 * self.n), actions=self._buf(ctypes.c_uint8, 8 * self.n),
                         rewards=self._buf(ctypes.c_double, 8 * self.n), flags=self._buf(ctypes.c_uint8, 8 * self.n),
                         probs=None, **self.out)
        self.args = dict(size=5, script=L.Script(L.SCRIPT_PRIORITY, (ctypes.c_uint8 * 4)(0, 1, 3, 2)), cfg=self.cfg,
                         env_state=u64(2 * self.n), env_inc=u64(2 * self.n), env_buf=u64(self.n),
                         pol_state=u64(2 * self.n), pol_inc=u64(2 * self.n), pol_buf=u64(self.n),
                         queue=self._buf(ctypes.c_uint32, 1), order=self._buf(ctypes.c_int32, self.n), n_order=self.n,
                         resume=0, sus=self.sus, n=self.n, cap=8, out=self.out, traj=self.traj, board_stride=8 * self.n,
                         max_workgroups=0, stream=None)

    def _buf(self, ctype, k):
        b = (ctype * k)()
        self.keep.append(b)
        return ctypes.addressof(b)

    def __call__(self, sus_over=None, out_over=None, **over):
        a = dict(self.args, **over)
        L = self.L
        s = L.Suspend(**dict(self.sus, **(sus_over or {})))
        byref = lambda x: ctypes.byref(x) if x is not None else None
        rows = self.which in ("rollout", "sized_rollout")
        if rows:
            o = L.Traj(**dict(self.traj, **(out_over or {})))
            outp = byref(o) if a["traj"] is not None else None
        else:
            o = L.EvalOut(**dict(self.out, **(out_over or {})))
            outp = byref(o) if a["out"] is not None else None
        susp = byref(s) if a["sus"] is not None else None
        head = (byref(a["script"]), byref(a["cfg"]), a["env_state"], a["env_inc"], a["env_buf"], a["pol_state"],
                a["pol_inc"], a["pol_buf"], a["queue"], a["order"], a["n_order"], a["resume"], susp, a["n"], a["cap"], outp)
        lib = L.lib()
        if self.which == "rollout":
            return lib.g2048_scripted_rollout(*head, a["max_workgroups"], a["stream"])
        if self.which == "eval":
            return lib.g2048_scripted_eval(*head, a["max_workgroups"], a["stream"])
        if self.which == "sized_rollout":
            return lib.g2048_sized_scripted_rollout(a["size"], *head, a["board_stride"], a["max_workgroups"], a["stream"])
        return lib.g2048_sized_scripted_eval(a["size"], *head, a["max_workgroups"], a["stream"])


FAMILIES = ("rollout", "eval", "sized_rollout", "sized_eval")


@pytest.fixture(scope="module")
def calls():
    from rl2048_amd import _lib as L

    return {w: _Call(L, w) for w in FAMILIES}


def _script(kind, order=(0, 1, 3, 2)):
    from rl2048_amd import _lib as L

    return L.Script(kind, (ctypes.c_uint8 * 4)(*order))


def _ids(o):
    return ",".join(f"{k}={'NULL' if v is None else v if isinstance(v, int) else 'obj'}" for k, v in o.items())


@pytest.mark.parametrize("which", FAMILIES)
def test_zero_count_returns_ok_without_a_launch(calls, which):
    call = calls[which]
    assert call(n_order=0) == call.L.G2048_OK
    assert call(n_order=0, order=None, n=0) == call.L.G2048_OK
    assert call(n_order=0, script=_script(UNIFORM, (9, 9, 9, 9))) == call.L.G2048_OK   # UNIFORM does not read order


COMMON = [dict(script=None), dict(script=_script(2)), dict(script=_script(-1)), dict(script=_script(PRIORITY, (0, 1, 2, 2))),
          dict(script=_script(PRIORITY, (0, 1, 2, 4))), dict(script=_script(PRIORITY, (1, 1, 1, 1))), dict(cfg=None),
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
def test_priority_without_action_mask_and_bad_cfg_are_einval(calls, which):
    call = calls[which]
    L = call.L
    cfg = L.EnvCfg.from_buffer_copy(call.cfg)
    cfg.use_action_mask = 0
    assert call(cfg=cfg) == L.G2048_EINVAL and b"use_action_mask" in L.lib().g2048_last_error()
    assert call(cfg=cfg, script=_script(UNIFORM), n_order=0) == L.G2048_OK      # UNIFORM plays without a mask
    cfg = L.EnvCfg.from_buffer_copy(call.cfg)
    cfg.reward_mode = 5
    assert call(cfg=cfg) == L.G2048_EINVAL


@pytest.mark.parametrize("which", ["rollout", "sized_rollout"])
def test_probs_and_null_row_buffers_are_einval(calls, which):
    call = calls[which]
    L = call.L
    assert call(out_over={"probs": call._buf(ctypes.c_float, 4 * 8 * call.n)}) == L.G2048_EINVAL
    assert b"probs" in L.lib().g2048_last_error()
    for field in ("boards", "actions", "rewards", "flags", "lengths", "totals", "max_tile", "final_board"):
        assert call(out_over={field: None}) == L.G2048_EINVAL, field


@pytest.mark.parametrize("which", ["eval", "sized_eval"])
def test_null_out_member_is_einval(calls, which):
    for field in ("lengths", "totals", "max_tile", "final_board"):
        assert calls[which](out_over={field: None}) == calls[which].L.G2048_EINVAL, field


@pytest.mark.parametrize("field", ["board", "meta", "total", "list", "count"])
@pytest.mark.parametrize("which", FAMILIES)
def test_null_suspend_member_is_einval(calls, which, field):
    assert calls[which](sus_over={field: None}) == calls[which].L.G2048_EINVAL


# --------------------------------------------------------------------------------------------------- Python
def test_priority_policy_validation():
    from rl2048_amd import PriorityPolicy, UniformPolicy

    assert PriorityPolicy([3, 0, 2, 1]).order == (3, 0, 2, 1)
    assert PriorityPolicy(np.array([0, 1, 3, 2])).order == PriorityPolicy.URLD
    for bad in ((0, 1, 2), (0, 1, 2, 3, 3), (0, 1, 2, 2), (0, 1, 2, 4), (-1, 0, 1, 2), (0.0, 1.0, 2.0, 3.0), "0123", 7,
                None):
        with pytest.raises(ValueError):
            PriorityPolicy(bad)
    assert callable(PriorityPolicy(URLD)) and not callable(UniformPolicy())
    with pytest.raises(TypeError):
        PriorityPolicy(URLD)(None, None)           # the reference hands None on a mask-less env: the caller falls back
    s = PriorityPolicy((2, 3, 0, 1))._script()
    assert s.kind == PRIORITY and list(s.order) == [2, 3, 0, 1] and UniformPolicy()._script().kind == UNIFORM


def _bare_agent(**env_kw):
    """A ReinforceAgent without a device: the refusals below must come before any device call reads one."""
    from rl2048_amd import Game2048EnvConfig
    from rl2048_amd.agent import ReinforceAgent

    a = object.__new__(ReinforceAgent)
    a.env_config = Game2048EnvConfig(**env_kw)
    a._sized = a.env_config.size != 4
    a._paths = {}
    return a


@pytest.mark.parametrize("method", ["rollout_batch", "evaluate_batch"])
def test_refusals_precede_any_device_call(method):
    from rl2048_amd import PriorityPolicy, UniformPolicy

    play = getattr(_bare_agent(), method)
    with pytest.raises(TypeError, match="run_episode"):
        play([1], [2], action_gen=lambda s, m: 0)
    with pytest.raises(ValueError, match="pcg64"):
        play([1], [2], rng="philox", action_gen=UniformPolicy())
    with pytest.raises(ValueError, match="use_action_mask"):
        getattr(_bare_agent(use_action_mask=False), method)([1], [2], action_gen=PriorityPolicy(URLD))
    with pytest.raises(ValueError, match="same length"):
        play([1], [2, 3], action_gen=UniformPolicy())
    if method == "rollout_batch":
        with pytest.raises(ValueError, match="record_probs"):
            play([1], [2], record_probs=True, action_gen=PriorityPolicy(URDL))
    assert _bare_agent()._paths == {}


def test_signatures_keep_their_defaults():
    import inspect

    from rl2048_amd import runner
    from rl2048_amd.agent import ReinforceAgent

    for f in (ReinforceAgent.rollout_batch, ReinforceAgent.evaluate_batch, runner.evaluation_loop):
        assert inspect.signature(f).parameters["action_gen"].default is None
    assert list(inspect.signature(ReinforceAgent.rollout_batch).parameters)[:7] == [
        "self", "env_seeds", "policy_seeds", "use_greedy", "rng", "check_every", "record_probs"]
    assert vars(ReinforceAgent)["scripted_max_workgroups"] == 0 and vars(ReinforceAgent)["scripted_rollout_cap0"] == 512
