"""CPU: the C ABI of the fused gradient for board sizes 2..8 (g2048_sized_grad, g2048_sized_onehot_dw1 and their
size queries, include/g2048_sized.h): declared as int, bound, exported, still ABI 17; every argument check returns
G2048_EINVAL before any HIP call (so it runs here, on host buffers that are never dereferenced); n == 0 returns
G2048_OK without a launch; the slab layout query agrees with the agent's unpacking for every size; nets past the
one-launch budget are refused; and the agent's switch is a class-level default that is off.  The kernels are tested
on the GPU in tests/test_gpu_sized_grad.py."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"g2048_sized_grad_slab": 4, "g2048_sized_grad_parts": 4, "g2048_sized_grad_layout": 8, "g2048_sized_grad": 25,
         "g2048_sized_onehot_dw1_slab": 2, "g2048_sized_onehot_dw1": 11}


def _harr(h):
    return (ctypes.c_int32 * len(h))(*h)


def test_entry_points_declared_bound_and_exported():
    from rl2048_amd import _lib

    assert _lib.ABI_VERSION == 17
    hdr = open(os.path.join(ROOT, "include", "g2048.h")).read()
    assert "#define G2048_ABI_VERSION 17" in hdr
    sized = open(os.path.join(ROOT, "include", "g2048_sized.h")).read()
    assert any(s.endswith("g2048_sized_grad.hip") for s in _lib.SOURCES)
    assert os.path.exists(_lib.LIB_PATH), "build() has run: the package is importable"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert _lib.lib().g2048_abi_version() == 17
    for name, nargs in NAMES.items():
        assert name not in hdr
        assert name in _lib.SIZED_SYMBOLS
        assert f"int {name}(" in sized
        assert f" T {name}" in out
        fn = getattr(_lib.lib(), name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name


class _Call:
    """g2048_sized_grad on small host buffers: valid arguments by default, one of them replaced per case."""

    def __init__(self, L):
        self.L = L
        self.keep = []
        f32 = lambda k: self._buf(ctypes.c_float, k)   # noqa: E731
        self.args = dict(size=5, packed=f32(16), grad_packed=f32(16), n_hidden=2, hidden=_harr([48, 16]),
                         activation=L.ACT_RELU, obs_mode=L.OBS_LOG2, obs_scale=0.125, use_mask=1,
                         boards=self._buf(ctypes.c_uint64, 2 * 8), plane_stride=8, actions=self._buf(ctypes.c_uint8, 8),
                         coef=f32(8), critic=0, loss=0, huber_delta=1.0, target=f32(8), delta_out=None, value_out=None,
                         d0_out=f32(8 * 64), hidden_out=None, n=8, partials=f32(64), nparts=2, stream=None)

    def _buf(self, ctype, k):
        b = (ctype * k)()
        self.keep.append(b)
        return ctypes.addressof(b)

    def __call__(self, **over):
        a = dict(self.args, **over)
        return self.L.lib().g2048_sized_grad(*[a[k] for k in self.args])


@pytest.fixture(scope="module")
def call():
    from rl2048_amd import _lib as L

    return _Call(L)


def test_n_zero_returns_ok_without_a_launch(call):
    """Valid arguments and no sample: G2048_OK, and (no device here) no HIP call was needed to say so."""
    L = call.L
    assert call(n=0) == L.G2048_OK
    assert call(n=0, plane_stride=0, boards=None, coef=None, actions=None, target=None, d0_out=None) == L.G2048_OK
    assert call(n=0, critic=1, loss=1, obs_mode=L.OBS_ONEHOT) == L.G2048_OK


@pytest.mark.parametrize("over", [
    dict(size=1), dict(size=9), dict(size=0), dict(size=-4),
    dict(plane_stride=7), dict(plane_stride=0),
    dict(n=-1), dict(n=(1 << 30) + 1, plane_stride=1 << 31),
    # a net the one launch does not cover
    dict(hidden=_harr([300, 16])), dict(hidden=_harr([48, 0])), dict(n_hidden=0), dict(n_hidden=5), dict(hidden=None),
    dict(n_hidden=3, hidden=_harr([256, 256, 256])), dict(n_hidden=2, hidden=_harr([256, 160])),
    dict(n_hidden=3, hidden=_harr([256, 160, 64]), obs_mode=2),
    dict(activation=7), dict(activation=-1), dict(obs_mode=-1), dict(obs_mode=3),
    dict(critic=1, loss=2), dict(critic=1, loss=-1),
    dict(nparts=0), dict(nparts=65536), dict(nparts=-3),
    # a NULL required buffer
    dict(packed=None), dict(partials=None), dict(grad_packed=None), dict(boards=None), dict(coef=None),
    dict(actions=None), dict(critic=1, target=None), dict(obs_mode=2, d0_out=None),
], ids=lambda o: ",".join(f"{k}={'NULL' if v is None else v if isinstance(v, int) else 'arr'}" for k, v in o.items()))
def test_einval_before_any_launch(call, over):
    L = call.L
    assert call(**over) == L.G2048_EINVAL
    assert L.lib().g2048_last_error()


def test_one_hidden_layer_needs_no_backward_fragments(call):
    """A one-layer net has no dense backward fragments: grad_packed may be NULL (here with n == 0, so no launch)."""
    assert call(n_hidden=1, hidden=_harr([48]), grad_packed=None, n=0) == call.L.G2048_OK


NETS = [[48], [1], [256], [64, 48, 32], [40, 33, 20, 10], [32, 16], [128, 64], [256, 128], [256, 128, 64]]


@pytest.mark.parametrize("size", range(2, 9))
def test_slab_layout_matches_the_agents_mirror(size):
    from rl2048_amd import _lib as L
    from rl2048_amd.agent import ReinforceAgent

    lib = L.lib()
    for mode in (L.OBS_RAW, L.OBS_LOG2, L.OBS_ONEHOT):
        onehot = mode == L.OBS_ONEHOT
        for hidden in NETS:
            nh, Hp = len(hidden), [32 * ((h + 31) // 32) for h in hidden]
            tiles = sum(Hp[l - 1] * Hp[l] // 1024 for l in range(1, nh))
            slab = lib.g2048_sized_grad_slab(size, mode, nh, _harr(hidden))
            if tiles > (40 if onehot else 32):
                assert slab == -1 and lib.g2048_sized_grad_parts(size, mode, nh, _harr(hidden)) == -1
                continue
            w_off, b_off = (ctypes.c_int32 * (nh + 1))(), (ctypes.c_int32 * (nh + 1))()
            rows, ld = ctypes.c_int32(-7), ctypes.c_int32(-7)
            got = lib.g2048_sized_grad_layout(size, mode, nh, _harr(hidden), w_off, b_off, ctypes.byref(rows),
                                              ctypes.byref(ld))
            pw, pb, rows0, total = ReinforceAgent._sized_slab_layout(size, hidden, onehot)
            assert got == slab == total > 0, (size, mode, hidden)
            assert list(w_off) == pw and list(b_off) == pb
            assert rows.value == rows0 and ld.value == Hp[0]
            assert rows0 == 0 if onehot else (rows0 >= size * size and rows0 % 32 == 0)
            # every segment inside the slab, in order, none overlapping
            sizes_w = [rows0 * Hp[0]] + [Hp[l - 1] * Hp[l] for l in range(1, nh)] + [Hp[-1] * 4]
            sizes_b = Hp + [4]
            off = 0
            for l in range(nh + 1):
                assert pw[l] == off
                off += sizes_w[l]
                assert pb[l] == off
                off += sizes_b[l]
            assert off == total
            assert lib.g2048_sized_grad_layout(size, mode, nh, _harr(hidden), None, None, None, None) == slab


def test_queries_refuse_what_is_not_covered():
    from rl2048_amd import _lib as L

    lib = L.lib()
    for q in (lib.g2048_sized_grad_slab, lib.g2048_sized_grad_parts):
        assert q(1, L.OBS_LOG2, 1, _harr([32])) == -1 and q(9, L.OBS_LOG2, 1, _harr([32])) == -1
        assert q(5, L.OBS_NONE, 1, _harr([32])) == -1
        assert q(5, L.OBS_LOG2, 0, _harr([32])) == -1 and q(5, L.OBS_LOG2, 1, None) == -1
        assert q(5, L.OBS_LOG2, 3, _harr([256, 256, 256])) == -1     # 128 tiles
        assert q(5, L.OBS_LOG2, 2, _harr([256, 129])) == -1          # 40 tiles: past raw / log2's 32
        assert q(5, L.OBS_RAW, 3, _harr([256, 128, 64])) == -1
        assert q(5, L.OBS_ONEHOT, 3, _harr([256, 129, 64])) == -1    # 8 x 5 + 5 x 2 = 50 tiles
    assert lib.g2048_sized_grad_slab(5, L.OBS_ONEHOT, 3, _harr([256, 128, 64])) > 0   # 40 tiles: the budget's edge
    assert lib.g2048_sized_grad_slab(5, L.OBS_ONEHOT, 2, _harr([256, 160])) > 0       # 40 tiles
    assert lib.g2048_sized_grad_slab(8, L.OBS_LOG2, 2, _harr([256, 128])) > 0         # 32 tiles
    assert lib.g2048_sized_grad_slab(4, L.OBS_RAW, 4, _harr([64, 64, 64, 64])) > 0    # size 4 is accepted


def test_onehot_dw1_slab_and_argument_checks():
    from rl2048_amd import _lib as L

    lib = L.lib()
    for size in range(2, 9):
        for h1 in (1, 33, 256):
            assert lib.g2048_sized_onehot_dw1_slab(size, h1) == (17 * size * size + 1) * h1
    for size, h1 in ((1, 32), (9, 32), (5, 0), (5, 257)):
        assert lib.g2048_sized_onehot_dw1_slab(size, h1) == -1
    keep = [(ctypes.c_uint64 * 64)(), (ctypes.c_float * 1024)(), (ctypes.c_float * 16)()]
    b, d1, part = (ctypes.addressof(k) for k in keep)
    ok = dict(size=5, boards=b, plane_stride=16, d1=d1, h1=32, m=16, ld=32, per=8, partials=part, nparts=2, stream=None)

    def call(**over):
        a = dict(ok, **over)
        return lib.g2048_sized_onehot_dw1(*[a[k] for k in ok])

    assert call(m=0, nparts=0) == L.G2048_OK
    for over in (dict(size=1), dict(size=9), dict(plane_stride=15), dict(h1=0), dict(h1=257), dict(m=-1),
                 dict(ld=31), dict(per=0), dict(nparts=1), dict(nparts=3), dict(boards=None), dict(d1=None),
                 dict(partials=None), dict(m=1 << 31, plane_stride=1 << 32, nparts=1, per=1 << 31),
                 dict(per=1 << 25, ld=32, m=1 << 26, plane_stride=1 << 26, nparts=2),
                 dict(m=1 << 20, plane_stride=1 << 20, per=8, nparts=1 << 17)):
        assert call(**over) == L.G2048_EINVAL, over
        assert lib.g2048_last_error()


def test_switch_is_a_class_level_default_that_is_off():
    from rl2048_amd.agent import ReinforceAgent

    assert ReinforceAgent.use_fused_sized_grad is False
    assert "use_fused_sized_grad" in vars(ReinforceAgent)
