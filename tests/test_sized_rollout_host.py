"""CPU: the C ABI of the persistent whole-rollout kernel for board sizes 2..8 (g2048_sized_rollout,
include/g2048_sized.h): declared, bound, exported, still ABI 17; every argument check returns G2048_EINVAL before any
HIP call (so it runs here, on host buffers that are never dereferenced); n_order == 0 returns G2048_OK without a
launch; and the agent's switch is a class-level default that is off.  The kernel itself is tested on the GPU in
tests/test_gpu_sized_rollout.py."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "g2048_sized_rollout"


def test_entry_point_declared_bound_and_exported():
    from rl2048_amd import _lib

    assert _lib.ABI_VERSION == 17
    hdr = open(os.path.join(ROOT, "include", "g2048.h")).read()
    assert "#define G2048_ABI_VERSION 17" in hdr and NAME not in hdr
    sized = open(os.path.join(ROOT, "include", "g2048_sized.h")).read()
    assert NAME in _lib.SIZED_SYMBOLS
    assert f"int {NAME}(" in sized
    assert any(s.endswith("g2048_sized_rollout.hip") for s in _lib.SOURCES)
    assert os.path.exists(_lib.LIB_PATH), "build() has run: the package is importable"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert f" T {NAME}" in out
    assert _lib.lib().g2048_abi_version() == 17
    fn = getattr(_lib.lib(), NAME)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 24


class _Call:
    """g2048_sized_rollout on small host buffers: valid arguments by default, one of them replaced per case."""

    def __init__(self, L):
        self.L = L
        self.n, self.cap = 4, 8
        self.keep = []
        u64 = lambda k: self._buf(ctypes.c_uint64, k)
        self.hidden = (ctypes.c_int32 * 2)(48, 16)
        self.cfg = L.EnvCfg(obs_mode=L.OBS_LOG2, reward_mode=1, bonus_mode=0, use_action_mask=1, obs_log2_scale=0.125,
                            base_reward_scale=1.0, invalid_action_penalty=-1.0, max_steps=8)
        self.sus = dict(board=u64(4 * self.n), meta=self._buf(ctypes.c_uint32, 3 * self.n),
                        total=self._buf(ctypes.c_double, self.n), list=self._buf(ctypes.c_int32, self.n),
                        count=self._buf(ctypes.c_uint32, 1))
        self.traj = dict(boards=u64(4 * self.cap * self.n), actions=self._buf(ctypes.c_uint8, self.cap * self.n),
                         rewards=self._buf(ctypes.c_double, self.cap * self.n),
                         flags=self._buf(ctypes.c_uint8, self.cap * self.n), probs=None,
                         lengths=self._buf(ctypes.c_int32, self.n), totals=self._buf(ctypes.c_double, self.n),
                         max_tile=self._buf(ctypes.c_uint8, self.n), final_board=u64(4 * self.n))
        self.args = dict(size=5, packed=self._buf(ctypes.c_float, 16), n_hidden=2, hidden=self.hidden,
                         activation=L.ACT_RELU, cfg=self.cfg, greedy=0, env_state=u64(2 * self.n),
                         env_inc=u64(2 * self.n), env_buf=u64(self.n), pol_state=u64(2 * self.n),
                         pol_inc=u64(2 * self.n), pol_buf=u64(self.n), queue=self._buf(ctypes.c_uint32, 1),
                         order=self._buf(ctypes.c_int32, self.n), n_order=self.n, resume=0, sus=self.sus, n=self.n,
                         cap=self.cap, traj=self.traj, board_stride=self.cap * self.n, max_workgroups=0, stream=None)

    def _buf(self, ctype, k):
        b = (ctype * k)()
        self.keep.append(b)
        return ctypes.addressof(b)

    def __call__(self, sus_over=None, traj_over=None, **over):
        a = dict(self.args, **over)                      # sus=None / traj=None in `over`: a NULL struct pointer
        s = self.L.Suspend(**dict(self.sus, **(sus_over or {})))
        t = self.L.Traj(**dict(self.traj, **(traj_over or {})))
        cfg = a["cfg"]
        return self.L.lib().g2048_sized_rollout(
            a["size"], a["packed"], a["n_hidden"], a["hidden"], a["activation"],
            ctypes.byref(cfg) if cfg is not None else None, a["greedy"], a["env_state"], a["env_inc"], a["env_buf"],
            a["pol_state"], a["pol_inc"], a["pol_buf"], a["queue"], a["order"], a["n_order"], a["resume"],
            ctypes.byref(s) if a["sus"] is not None else None, a["n"], a["cap"],
            ctypes.byref(t) if a["traj"] is not None else None, a["board_stride"], a["max_workgroups"], a["stream"])


@pytest.fixture(scope="module")
def call():
    from rl2048_amd import _lib as L

    return _Call(L)


def test_n_order_zero_returns_ok_without_a_launch(call):
    """Valid arguments and nothing to play: G2048_OK, and (no device here) no HIP call was needed to say so."""
    L = call.L
    assert call(n_order=0) == L.G2048_OK
    assert call(n_order=0, order=None, n=0, board_stride=0) == L.G2048_OK


@pytest.mark.parametrize("over", [
    dict(size=1), dict(size=9), dict(size=0),
    # a net g2048_sized_policy_packed_size does not cover
    dict(hidden=(ctypes.c_int32 * 2)(300, 16)), dict(hidden=(ctypes.c_int32 * 2)(48, 0)), dict(n_hidden=0),
    dict(n_hidden=5), dict(hidden=None), dict(activation=7),
    # board_stride < cap * n
    dict(board_stride=4 * 8 - 1), dict(board_stride=0),
    # n / cap / order: g2048_deep_rollout's rules
    dict(n=-1), dict(n=1 << 31), dict(n_order=-1), dict(n_order=5), dict(order=None, n_order=3),
    dict(order=None, resume=1), dict(cap=0), dict(cap=1 << 31), dict(n=1 << 21, n_order=4, cap=(1 << 20) + 1,
                                                                  board_stride=1 << 62),
    dict(max_workgroups=-1),
    # a NULL required buffer
    dict(packed=None), dict(env_state=None), dict(env_inc=None), dict(env_buf=None), dict(pol_state=None),
    dict(pol_inc=None), dict(pol_buf=None), dict(queue=None), dict(sus=None), dict(traj=None), dict(cfg=None),
], ids=lambda o: ",".join(f"{k}={'NULL' if v is None else v if isinstance(v, int) else 'arr'}" for k, v in o.items()))
def test_einval_before_any_launch(call, over):
    L = call.L
    assert call(**over) == L.G2048_EINVAL
    assert L.lib().g2048_last_error()


@pytest.mark.parametrize("where,field", [("sus", f) for f in ("board", "meta", "total", "list", "count")] +
                         [("traj", f) for f in ("boards", "actions", "rewards", "flags", "lengths", "totals",
                                                "max_tile", "final_board")])
def test_null_struct_member_is_einval(call, where, field):
    assert call(**{where + "_over": {field: None}}) == call.L.G2048_EINVAL


def test_obs_mode_the_packed_net_does_not_cover_is_einval(call):
    L = call.L
    cfg = L.EnvCfg.from_buffer_copy(call.cfg)
    cfg.obs_mode = L.OBS_NONE
    assert call(cfg=cfg) == L.G2048_EINVAL


def test_switch_is_a_class_level_default_that_is_off():
    from rl2048_amd.agent import ReinforceAgent

    assert ReinforceAgent.use_fused_sized_rollout is False
    assert "use_fused_sized_rollout" in vars(ReinforceAgent)
    assert ReinforceAgent.sized_rollout_max_workgroups == 0
    assert ReinforceAgent.sized_rollout_cap0 == 512
    assert ReinforceAgent.sized_rollout_max_rows == 1 << 24
