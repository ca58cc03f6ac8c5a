"""CPU: the C ABI of the score-only rollouts (g2048_rollout_eval and g2048_deep_eval, include/g2048_eval.h;
g2048_sized_eval, include/g2048_sized.h): declared, bound, exported, still ABI 17; every argument check returns
G2048_EINVAL before any HIP call (so it runs here, on host buffers that are never dereferenced); the zero-count calls
return G2048_OK without a launch; and the agent's side exists with its class-level defaults.  The kernels themselves
are tested on the GPU in tests/test_gpu_eval.py."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = {"g2048_rollout_eval": 16, "g2048_deep_eval": 21, "g2048_sized_eval": 23}


def test_entry_points_declared_bound_and_exported():
    from rl2048_amd import _lib

    assert _lib.ABI_VERSION == 17
    hdr = open(os.path.join(ROOT, "include", "g2048.h")).read()
    assert "#define G2048_ABI_VERSION 17" in hdr and '#include "g2048_eval.h"' in hdr
    ev = open(os.path.join(ROOT, "include", "g2048_eval.h")).read()
    sized = open(os.path.join(ROOT, "include", "g2048_sized.h")).read()
    assert "typedef struct g2048_eval_out" in ev
    assert _lib.EVAL_SYMBOLS == ("g2048_rollout_eval", "g2048_deep_eval")
    for name in _lib.EVAL_SYMBOLS:
        assert f"int {name}(" in ev and f"int {name}(" not in hdr and name not in _lib.EXPORTED_SYMBOLS
    assert "g2048_sized_eval" in _lib.SIZED_SYMBOLS and "int g2048_sized_eval(" in sized
    for tu in ("g2048_rollout_eval.hip", "g2048_sized_eval.hip"):
        assert any(s.endswith(tu) for s in _lib.SOURCES)
    assert os.path.exists(_lib.LIB_PATH), "build() has run: the package is importable"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    lib = _lib.lib()
    assert lib.g2048_abi_version() == 17
    for name, nargs in NARGS.items():
        assert f" T {name}" in out
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
    assert [f for f, _ in _lib.EvalOut._fields_] == ["lengths", "totals", "max_tile", "final_board"]
    assert ctypes.sizeof(_lib.EvalOut) == 4 * ctypes.sizeof(ctypes.c_void_p)


class _Call:
    """One of the three entry points on small host buffers: valid arguments by default, one replaced per case."""

    def __init__(self, L, which):
        self.L, self.which = L, which
        self.n = 4
        self.keep = []
        u64 = lambda k: self._buf(ctypes.c_uint64, k)
        self.hidden = (ctypes.c_int32 * 2)(48, 16)
        self.cfg = L.EnvCfg(obs_mode=L.OBS_LOG2, reward_mode=1, bonus_mode=0, use_action_mask=1, obs_log2_scale=0.125,
                            base_reward_scale=1.0, invalid_action_penalty=-1.0, max_steps=8)
        self.sus = dict(board=u64(4 * self.n), meta=self._buf(ctypes.c_uint32, 3 * self.n),
                        total=self._buf(ctypes.c_double, self.n), list=self._buf(ctypes.c_int32, self.n),
                        count=self._buf(ctypes.c_uint32, 1))
        self.out = dict(lengths=self._buf(ctypes.c_int32, self.n), totals=self._buf(ctypes.c_double, self.n),
                        max_tile=self._buf(ctypes.c_uint8, self.n), final_board=u64(4 * self.n))
        self.args = dict(size=5, packed=self._buf(ctypes.c_float, 16), h1=48, h2=16, n_hidden=2, hidden=self.hidden,
                         activation=L.ACT_RELU, cfg=self.cfg, greedy=0, env_state=u64(2 * self.n),
                         env_inc=u64(2 * self.n), env_buf=u64(self.n), pol_state=u64(2 * self.n),
                         pol_inc=u64(2 * self.n), pol_buf=u64(self.n), queue=self._buf(ctypes.c_uint32, 1),
                         order=self._buf(ctypes.c_int32, self.n), n_order=self.n, resume=0, sus=self.sus, n=self.n,
                         step_limit=8, out=self.out, max_workgroups=0, stream=None)

    def _buf(self, ctype, k):
        b = (ctype * k)()
        self.keep.append(b)
        return ctypes.addressof(b)

    def __call__(self, sus_over=None, out_over=None, **over):
        a = dict(self.args, **over)                      # sus=None / out=None in `over`: a NULL struct pointer
        s = self.L.Suspend(**dict(self.sus, **(sus_over or {})))
        o = self.L.EvalOut(**dict(self.out, **(out_over or {})))
        cfg = a["cfg"]
        cfgp = ctypes.byref(cfg) if cfg is not None else None
        outp = ctypes.byref(o) if a["out"] is not None else None
        susp = ctypes.byref(s) if a["sus"] is not None else None
        streams = (a["env_state"], a["env_inc"], a["env_buf"], a["pol_state"], a["pol_inc"], a["pol_buf"], a["queue"])
        lib = self.L.lib()
        if self.which == "rollout":
            return lib.g2048_rollout_eval(a["packed"], a["h1"], a["h2"], a["activation"], cfgp, a["greedy"], *streams,
                                          a["n"], outp, a["stream"])
        tail = (a["order"], a["n_order"], a["resume"], susp, a["n"], a["step_limit"], outp)
        if self.which == "deep":
            return lib.g2048_deep_eval(a["packed"], a["n_hidden"], a["hidden"], a["activation"], cfgp, a["greedy"],
                                       *streams, *tail, a["stream"])
        return lib.g2048_sized_eval(a["size"], a["packed"], a["n_hidden"], a["hidden"], a["activation"], cfgp,
                                    a["greedy"], *streams, *tail, a["max_workgroups"], a["stream"])


FAMILIES = ("rollout", "deep", "sized")
SUSPENDING_FAMILIES = ("deep", "sized")                  # the two-layer kernel has no suspend path


@pytest.fixture(scope="module")
def calls():
    from rl2048_amd import _lib as L

    return {w: _Call(L, w) for w in FAMILIES}


def _ids(o):
    return ",".join(f"{k}={'NULL' if v is None else v if isinstance(v, int) else 'arr'}" for k, v in o.items())


@pytest.mark.parametrize("which", FAMILIES)
def test_zero_count_returns_ok_without_a_launch(calls, which):
    """Valid arguments and nothing to play: G2048_OK, and (no device here) no HIP call was needed to say so."""
    call = calls[which]
    L = call.L
    if which == "rollout":
        assert call(n=0) == L.G2048_OK
    else:
        assert call(n_order=0) == L.G2048_OK
        assert call(n_order=0, order=None, n=0) == L.G2048_OK


STREAM_NULLS = [dict(packed=None), dict(env_state=None), dict(env_inc=None), dict(env_buf=None), dict(pol_state=None),
                dict(pol_inc=None), dict(pol_buf=None), dict(queue=None), dict(out=None), dict(cfg=None)]
# what the counterparts reject that still applies (n / order / net / activation rules), and step_limit < 1
SUSPENDING = [dict(n=-1), dict(n=1 << 31), dict(n_order=-1), dict(n_order=5), dict(order=None, n_order=3),
              dict(order=None, resume=1), dict(step_limit=0), dict(step_limit=-1), dict(step_limit=1 << 31),
              dict(hidden=(ctypes.c_int32 * 2)(300, 16)), dict(hidden=(ctypes.c_int32 * 2)(48, 0)), dict(n_hidden=0),
              dict(n_hidden=5), dict(hidden=None), dict(activation=7), dict(sus=None)]
CASES = {"rollout": [dict(n=-1), dict(n=1 << 31), dict(h1=0), dict(h2=300), dict(activation=7)] + STREAM_NULLS,
         "deep": SUSPENDING + STREAM_NULLS,
         "sized": SUSPENDING + STREAM_NULLS + [dict(size=1), dict(size=9), dict(size=0), dict(max_workgroups=-1)]}
EINVAL_CASES = [(w, c) for w in FAMILIES for c in CASES[w]]


@pytest.mark.parametrize("which,over", EINVAL_CASES, ids=[f"{w}-{_ids(c)}" for w, c in EINVAL_CASES])
def test_einval_before_any_launch(calls, which, over):
    L = calls[which].L
    assert calls[which](**over) == L.G2048_EINVAL
    assert L.lib().g2048_last_error()


@pytest.mark.parametrize("field", ["lengths", "totals", "max_tile", "final_board"])
@pytest.mark.parametrize("which", FAMILIES)
def test_null_out_member_is_einval(calls, which, field):
    assert calls[which](out_over={field: None}) == calls[which].L.G2048_EINVAL


@pytest.mark.parametrize("field", ["board", "meta", "total", "list", "count"])
@pytest.mark.parametrize("which", SUSPENDING_FAMILIES)
def test_null_suspend_member_is_einval(calls, which, field):
    assert calls[which](sus_over={field: None}) == calls[which].L.G2048_EINVAL


@pytest.mark.parametrize("which", FAMILIES)
def test_cfg_the_kernels_do_not_cover_is_einval(calls, which):
    call = calls[which]
    L = call.L
    cfg = L.EnvCfg.from_buffer_copy(call.cfg)
    if which == "rollout":
        cfg.obs_mode = L.OBS_ONEHOT                      # the two-layer family: log2 / raw only
        assert call(cfg=cfg) == L.G2048_EINVAL
        cfg = L.EnvCfg.from_buffer_copy(call.cfg)
        cfg.max_steps = -1                               # ... and bounded by a finite max_steps
        assert call(cfg=cfg) == L.G2048_EINVAL and b"max_steps" in L.lib().g2048_last_error()
    elif which == "sized":
        cfg.obs_mode = L.OBS_NONE
        assert call(cfg=cfg) == L.G2048_EINVAL
    cfg = L.EnvCfg.from_buffer_copy(call.cfg)
    cfg.reward_mode = 5
    assert call(cfg=cfg) == L.G2048_EINVAL


def test_agent_side_exists_with_class_level_defaults():
    import dataclasses
    import inspect

    from rl2048_amd.agent import EvalBatch, ReinforceAgent

    assert [f.name for f in dataclasses.fields(EvalBatch)] == ["lengths", "total_reward", "max_tile", "final_boards",
                                                               "shard_sizes"]
    assert isinstance(vars(EvalBatch)["n"], property)
    sig = inspect.signature(ReinforceAgent.evaluate_batch)
    assert list(sig.parameters)[:4] == ["self", "env_seeds", "policy_seeds", "use_greedy"]
    assert sig.parameters["use_greedy"].default is True
    assert vars(ReinforceAgent)["eval_step_budget"] == 4096
    assert vars(ReinforceAgent)["eval_max_steps"] == 1 << 20
    from rl2048_amd import runner

    p = inspect.signature(runner.evaluation_loop).parameters
    assert p["score_only"].default is False and p["chunk"].default == 65536
