"""CPU: the C ABI of the fused policy for board sizes 2..8 (g2048_sized_policy_packed_size / g2048_sized_pack /
g2048_sized_policy, include/g2048_sized.h): declared, bound, exported, still ABI 17, and the host-only shape check.
The kernel itself is tested on the GPU in tests/test_gpu_sized_policy.py."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("g2048_sized_policy_packed_size", "g2048_sized_pack", "g2048_sized_policy")


def test_entry_points_declared_bound_and_exported():
    from rl2048_amd import _lib

    assert _lib.ABI_VERSION == 17
    hdr = open(os.path.join(ROOT, "include", "g2048.h")).read()
    assert "#define G2048_ABI_VERSION 17" in hdr
    sized = open(os.path.join(ROOT, "include", "g2048_sized.h")).read()
    for s in NAMES:
        assert s in _lib.SIZED_SYMBOLS
        assert f"int {s}(" in sized
        assert s not in hdr                      # g2048.h's own list of functions is pinned by tests/test_capi.py
    if os.path.exists(_lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
        assert all(f" T {s}" in out for s in NAMES)
        assert _lib.lib().g2048_abi_version() == 17
        for s in NAMES:
            assert getattr(_lib.lib(), s).restype is ctypes.c_int


def _size(L, size, obs, hidden):
    harr = (ctypes.c_int32 * max(len(hidden), 1))(*hidden)
    return L.lib().g2048_sized_policy_packed_size(size, obs, len(hidden), harr)


def test_packed_size_covers_exactly_the_documented_shapes():
    """Host arithmetic only (no device is touched, so this runs without a GPU)."""
    from rl2048_amd import _lib as L

    ok = [64, 32]
    assert _size(L, 1, L.OBS_LOG2, ok) == -1
    assert _size(L, 9, L.OBS_LOG2, ok) == -1
    assert _size(L, 5, L.OBS_LOG2, []) == -1
    assert _size(L, 5, L.OBS_LOG2, [8, 8, 8, 8, 8]) == -1
    assert _size(L, 5, L.OBS_ONEHOT, [32, 0]) == -1
    assert _size(L, 5, L.OBS_ONEHOT, [257]) == -1
    assert _size(L, 5, L.OBS_NONE, ok) == -1
    assert L.lib().g2048_sized_policy_packed_size(5, L.OBS_LOG2, 2, None) == -1
    for size in range(2, 9):
        for obs in (L.OBS_RAW, L.OBS_LOG2, L.OBS_ONEHOT):
            for hidden in ([1], [7], [64, 64], [256, 128, 64], [256, 256, 256, 256], [40, 33, 20, 10]):
                assert _size(L, size, obs, hidden) > 0, (size, obs, hidden)


@pytest.mark.parametrize("size", range(2, 9))
def test_packed_size_is_the_documented_layout(size):
    """The float count of the layout in g2048_sized_policy.hip: layer 0 (raw / log2: nt0 x ceil(N*N / 2) k-steps x 64
    lanes; one-hot: nt0 x N*N cells x 3 planes x 64 lanes x 4 dwords), dense layers of 32 x 32 tiles, padded biases,
    the [units][4] output layer and its 4 biases."""
    from rl2048_amd import _lib as L

    cells = size * size
    for hidden in ([7], [64, 48], [256, 128, 64], [33, 100, 1, 256]):
        nt = [(h + 31) // 32 for h in hidden]
        rest = sum(32 * t for t in nt) + sum(a * b * 1024 for a, b in zip(nt[:-1], nt[1:])) + 32 * nt[-1] * 4 + 4
        assert _size(L, size, L.OBS_LOG2, hidden) == rest + nt[0] * ((cells + 1) // 2) * 64
        assert _size(L, size, L.OBS_RAW, hidden) == _size(L, size, L.OBS_LOG2, hidden)
        assert _size(L, size, L.OBS_ONEHOT, hidden) == rest + nt[0] * cells * 3 * 64 * 4
