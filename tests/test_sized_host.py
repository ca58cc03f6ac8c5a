"""CPU checks of the N x N board arithmetic the gfx950 sized kernels run (csrc/g2048_sized_core.h), through a
TEST-ONLY host build (tests/native/sized_host.cpp), against tests/golden/sized.npz (recorded from the real
reference by tests/golden/make_golden_sized.py) and the CPU oracle's Philox; plus the config layer's size handling.

Not a parity claim for the GPU path (that is tests/test_gpu_sized.py); it localises logic bugs on the CPU.
"""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "rl-2048-with-reinforce-and-actor-critic_amd", "csrc")
SIZES = [2, 3, 5, 6, 7, 8]

u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)


class EpCfg(ctypes.Structure):
    _fields_ = [("reward_mode", ctypes.c_int32), ("bonus_mode", ctypes.c_int32), ("use_action_mask", ctypes.c_int32),
                ("pad", ctypes.c_int32)] + [(k, ctypes.c_double) for k in (
                    "base_reward_scale", "empty_tile_reward", "merge_reward", "bonus_scale", "step_reward",
                    "endgame_penalty", "invalid_action_penalty")] + [("max_steps", ctypes.c_int64)]


def ep_cfg(kw) -> EpCfg:
    d = dict(reward_mode="sum", base_reward_scale=1.0, empty_tile_reward=0.0, merge_reward=0.0, bonus_mode="off",
             bonus_scale=1.0, step_reward=0.0, endgame_penalty=0.0, use_action_mask=True, invalid_action_penalty=-1.0,
             max_steps=1024)
    d.update({k: v for k, v in kw.items() if k in d})
    c = EpCfg()
    c.reward_mode = {"sum": 0, "log2": 1}[d["reward_mode"]]
    c.bonus_mode = {"off": 0, "raw": 1, "log2": 2}[d["bonus_mode"]]
    c.use_action_mask = int(d["use_action_mask"])
    for k in ("base_reward_scale", "empty_tile_reward", "merge_reward", "bonus_scale", "step_reward",
              "endgame_penalty", "invalid_action_penalty"):
        setattr(c, k, float(d[k]))
    c.max_steps = -1 if d["max_steps"] is None else int(d["max_steps"])
    return c


def _sources():
    return [os.path.join(NATIVE, "sized_host.cpp"), os.path.join(CSRC, "g2048_sized_core.h"),
            os.path.join(CSRC, "g2048_core.h")]


@pytest.fixture(scope="module")
def sh():
    so = os.path.join(NATIVE, "libsized_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in _sources()):
        tmp = f"{so}.{os.getpid()}.tmp"   # build aside, then rename: parallel workers never load a partial file
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-o", tmp, _sources()[0]],
                       check=True)
        os.replace(tmp, so)
    L = ctypes.CDLL(so)
    L.sh_line_move.restype = ctypes.c_uint32
    L.sh_line_move.argtypes = [ctypes.c_int, ctypes.c_uint32, u32p, u32p]
    L.sh_move.argtypes = [ctypes.c_int, u64p, ctypes.c_uint32, u64p, ctypes.c_void_p, u32p]
    L.sh_mask.restype = ctypes.c_uint32
    L.sh_mask.argtypes = [ctypes.c_int, u64p]
    L.sh_done.argtypes = [ctypes.c_int, u64p]
    L.sh_symmetry.argtypes = [ctypes.c_int, u64p, ctypes.c_int, u64p]
    L.sh_symmetry_action.restype = ctypes.c_uint32
    L.sh_symmetry_action.argtypes = [ctypes.c_uint32, ctypes.c_int]
    L.sh_philox.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, u32p]
    L.sh_spawn_philox.argtypes = [ctypes.c_int, u64p, ctypes.c_uint32, ctypes.c_uint32, u64p]
    L.sh_fresh_philox.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, u64p]
    L.sh_episode.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(EpCfg)] + \
        [ctypes.c_void_p] * 7 + [u32p]
    L.sh_episode_from.argtypes = [ctypes.c_int, ctypes.c_uint64, u64p, ctypes.c_void_p, ctypes.c_int64,
                                  ctypes.POINTER(EpCfg)] + [ctypes.c_void_p] * 7 + [u32p]
    L.sh_selfcheck.restype = ctypes.c_int64
    L.sh_selfcheck.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_uint64]
    L.sh_check_n4.restype = ctypes.c_int64
    L.sh_check_n4.argtypes = [ctypes.c_int64, ctypes.c_uint64]
    return L


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(ROOT, "tests", "golden", "sized.npz")) as z:
        return {k: z[k] for k in z.files}


def words(n):
    return (n * n + 15) // 16


def pack(e, n):
    """uint8 exponents [N*N] -> ctypes uint64[W] (cell k: nibble k & 15 of word k >> 4)."""
    w = [0] * words(n)
    for k, v in enumerate(np.asarray(e).reshape(-1).tolist()):
        w[k >> 4] |= int(v) << (4 * (k & 15))
    return (ctypes.c_uint64 * len(w))(*w)


def unpack(w, n):
    return np.array([(int(w[k >> 4]) >> (4 * (k & 15))) & 15 for k in range(n * n)], dtype=np.uint8)


@pytest.mark.parametrize("n", range(2, 9))
def test_lines_match_reference(sh, gold, n):
    lin, lout, lmer = gold[f"n{n}_line_in"], gold[f"n{n}_line_out"], gold[f"n{n}_line_merged"]
    assert len(lin) >= 3 ** n
    for a, b, m in zip(lin.tolist(), lout.tolist(), lmer.tolist()):
        line = sum(v << (4 * k) for k, v in enumerate(a))
        ml, s = ctypes.c_uint32(), (ctypes.c_uint32 * 4)()
        out = sh.sh_line_move(n, line, ctypes.byref(ml), s)
        got = [(out >> (4 * k)) & 15 for k in range(n)]
        assert got == [min(v, 15) for v in b], (a, got, b)        # 15+15 saturates at 15 on the board
        mer = [e for e in m if e]
        assert [(ml.value >> (8 * q)) & 255 for q in range(len(mer))] == mer and ml.value >> (8 * len(mer)) == 0
        assert list(s) == [len(mer), sum(mer), sum(1 << e for e in mer), max(mer, default=0)]


@pytest.mark.parametrize("n", SIZES)
def test_crafted_boards_mask_and_done(sh, gold, n):
    for e, m, d in zip(gold[f"n{n}_craft_board"], gold[f"n{n}_craft_mask"], gold[f"n{n}_craft_done"]):
        b = pack(e, n)
        assert sh.sh_mask(n, b) == int(m), e.reshape(n, n)
        assert bool(sh.sh_done(n, b)) == bool(d), e.reshape(n, n)


def test_n4_equals_bitboard_core(sh):
    # move (board, summary, merged list), action mask, is_done and the PCG64 spawn against g2048_core.h
    assert sh.sh_check_n4(200000, 12345) == 0


@pytest.mark.parametrize("n", range(2, 9))
def test_against_array_game(sh, n):
    # the fixture-free checks the sanitizer program also runs: a plain array implementation of the game
    assert sh.sh_selfcheck(n, 3000, 99 + n) == 0


@pytest.mark.parametrize("n", SIZES)
def test_fixture_episodes_replay(sh, gold, n):
    """Whole reference episodes from reset(seed): the PCG64 spawn stream, boards, flags, score, merged lists, masks,
    max_tile_seen and the fp64 reward bit for bit."""
    cfgs = json.loads(str(gold["env_cfgs"]))
    LEN = n * (n // 2)
    W = words(n)
    for c, kw in cfgs.items():
        p = f"n{n}_c{c}_"
        cfg = ep_cfg(kw)
        for e, (seed, start, ln) in enumerate(zip(gold[p + "ep_seed"], gold[p + "ep_start"], gold[p + "ep_len"])):
            ln, start = int(ln), int(start)
            acts = np.ascontiguousarray(gold[p + "action"][start:start + ln])
            boards = np.zeros((ln + 1, W), dtype=np.uint64)
            lists = np.zeros((ln, LEN), dtype=np.uint8)
            rewards = np.zeros(ln, dtype=np.float64)
            flags, sadd, masks, mt = (np.zeros(ln, dtype=np.uint32) for _ in range(4))
            rmask = ctypes.c_uint32()
            sh.sh_episode(n, int(seed), acts.ctypes.data, ln, ctypes.byref(cfg), boards.ctypes.data, lists.ctypes.data,
                          rewards.ctypes.data, flags.ctypes.data, sadd.ctypes.data, masks.ctypes.data, mt.ctypes.data,
                          ctypes.byref(rmask))
            assert np.array_equal(unpack(boards[0], n), gold[p + "reset_board"][e])
            assert rmask.value == int(gold[p + "reset_mask"][e])
            sl = slice(start, start + ln)
            got_boards = np.array([unpack(b, n) for b in boards[1:]])
            assert np.array_equal(got_boards, gold[p + "board"][sl]), (n, c, e)
            assert np.array_equal(lists, gold[p + "merged"][sl])
            assert np.array_equal(rewards.view(np.uint64), gold[p + "reward"][sl].view(np.uint64)), (n, c, e)
            assert np.array_equal((flags & 2) != 0, gold[p + "terminated"][sl])
            assert np.array_equal((flags & 4) != 0, gold[p + "truncated"][sl])
            assert np.array_equal((flags & 8) != 0, gold[p + "invalid"][sl])
            assert np.array_equal(np.cumsum(sadd.astype(np.int64)), gold[p + "score"][sl])
            assert np.array_equal(masks, gold[p + "mask"][sl])
            assert np.array_equal(np.int64(1) << mt.astype(np.int64), gold[p + "max_tile_seen"][sl])
            prev = np.concatenate([gold[p + "reset_board"][e][None], gold[p + "board"][sl][:-1]])
            assert np.array_equal((flags & 1) != 0, (prev != gold[p + "board"][sl]).any(axis=1))


@pytest.mark.parametrize("n", [3, 5])
def test_symmetries_match_reference(sh, gold, n):
    p = f"n{n}_s0_"          # log2 obs, scale 0.25: obs = exponent * 0.25
    for e, a, obs_out, act_out in zip(gold[p + "board_in"], gold[p + "action_in"], gold[p + "obs_out"],
                                      gold[p + "action_out"]):
        b = pack(e, n)
        for k in range(8):
            out = (ctypes.c_uint64 * words(n))()
            sh.sh_symmetry(n, b, k, out)
            assert np.array_equal(unpack(out, n).astype(np.float32) * np.float32(0.25), obs_out[k]), (n, k)
            assert sh.sh_symmetry_action(int(a), k) == int(act_out[k])


def test_philox_draw_and_spawn_rule(sh):
    """The Philox draw is Philox4x32-10 on counter (seed lo, seed hi, ctr, tag) keyed by the key's halves; a spawn
    puts a 2 (draw y < 0.9 * 2**32) or 4 into empty cell number (x * n_empty) >> 32 in row-major order."""
    rng = np.random.default_rng(5)
    for _ in range(200):
        key, seed = (int(v) for v in rng.integers(0, 2**63, size=2, dtype=np.uint64))
        ctr, tag = int(rng.integers(0, 2**20)), int(rng.integers(0, 4))
        out = (ctypes.c_uint32 * 4)()
        sh.sh_philox(key, seed, ctr, tag, out)
        ref = O.philox4x32_10((seed & 0xFFFFFFFF, seed >> 32, ctr, tag), (key & 0xFFFFFFFF, key >> 32))
        assert list(out) == [int(v) for v in ref]
    for n in range(2, 9):
        for _ in range(300):
            e = rng.integers(1, 12, size=n * n)
            e[rng.random(n * n) < rng.choice([0.1, 0.5, 0.95])] = 0
            if (e != 0).all():
                e[int(rng.integers(n * n))] = 0
            rx, ry = (int(v) for v in rng.integers(0, 2**32, size=2, dtype=np.uint64))
            out = (ctypes.c_uint64 * words(n))()
            sh.sh_spawn_philox(n, pack(e, n), rx, ry, out)
            empties = np.flatnonzero(e == 0)
            want = e.copy()
            want[empties[(rx * len(empties)) >> 32]] = 1 if ry < 3865470566 else 2
            assert np.array_equal(unpack(out, n), want.astype(np.uint8)), (n, e)
        # the reset board: counter 0, tag 1; x, y spawn the first tile, z, w the second
        key, seed = 0x2048, int(rng.integers(0, 2**62))
        d = (ctypes.c_uint32 * 4)()
        sh.sh_philox(key, seed, 0, 1, d)
        b1 = (ctypes.c_uint64 * words(n))()
        sh.sh_spawn_philox(n, pack(np.zeros(n * n, np.uint8), n), d[0], d[1], b1)
        b2 = (ctypes.c_uint64 * words(n))()
        sh.sh_spawn_philox(n, b1, d[2], d[3], b2)
        fresh = (ctypes.c_uint64 * words(n))()
        sh.sh_fresh_philox(n, key, seed, fresh)
        assert list(fresh) == list(b2)


def test_sanitizer_program():
    """The fixture-free checks as a stand-alone program (own main) under AddressSanitizer + UBSan: a shift count of
    64 or more in the multi-word nibble code is undefined behaviour that happens to work on one target."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = os.path.join(NATIVE, f"sized_host_san.{os.getpid()}")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-DSIZED_HOST_MAIN", "-I" + CSRC, "-o", exe, _sources()[0]], capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower() or "sanitize" in r.stderr.lower()):
        pytest.skip("the sanitizer runtimes are not installed: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr
    try:
        run = subprocess.run([exe], capture_output=True, text=True)
    finally:
        os.remove(exe)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "total: 0 mismatches" in run.stdout


# ---------------------------------------------------------------------------------------------------- config layer
def test_config_sizes():
    from rl2048_amd import Game2048EnvConfig
    from rl2048_amd.config import board_words, env_cfg_struct, obs_width

    for n in range(2, 9):
        env_cfg_struct(Game2048EnvConfig(size=n))
        assert obs_width("raw", n) == n * n and obs_width("log2", n) == n * n and obs_width("onehot", n) == n * n * 17
        assert board_words(n) == (n * n + 15) // 16
    assert [board_words(n) for n in range(2, 9)] == [1, 1, 1, 2, 3, 4, 4]
    assert obs_width("log2") == 16 and obs_width("onehot") == 272
    for bad in (1, 9, 0, -4, 4.0, None):
        with pytest.raises(ValueError):
            env_cfg_struct(Game2048EnvConfig(size=bad))
    with pytest.raises(ValueError):
        obs_width("log2", 9)


def test_abi_17_declares_sized_entry_points():
    from rl2048_amd import _lib

    assert _lib.ABI_VERSION == 17
    for s in ("g2048_sized_words", "g2048_sized_reset", "g2048_sized_step", "g2048_sized_obs", "g2048_sized_move",
              "g2048_sized_symmetries"):
        assert s in _lib.SIZED_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "g2048.h")).read()
    assert "#define G2048_ABI_VERSION 17" in hdr and "size is fixed at 4" not in hdr
    assert '#include "g2048_sized.h"' in hdr
    sized = open(os.path.join(ROOT, "include", "g2048_sized.h")).read()
    for s in _lib.SIZED_SYMBOLS:
        assert f"int {s}(" in sized
    # the built library exports them (build() has run: the package is importable)
    if os.path.exists(_lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
        assert all(f" T {s}" in out for s in _lib.SIZED_SYMBOLS)
