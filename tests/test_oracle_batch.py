"""The batched oracle (oracle.EnvBatch: one C call per step, OpenMP over lanes) equals the per-lane oracle (O.Env)
bit for bit on every output, so the GPU tests that compare every lane of a large batch against EnvBatch
(tests/test_gpu_step_matrix.py) stand on the oracle the golden fixtures pin (tests/test_oracle_golden.py,
tests/test_oracle_ref_fixtures.py).

The lane bookkeeping EnvBatch adds -- inactive lanes, actions > 3, auto-reset with seed += stride -- is restated
here in Python around O.Env, independently of the C loop."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_env import ENV_CFGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T, STRIDE, KEY = 200, 40, 1000, 0x5EED2048
UNREP_LANE = 5           # holds two 2**15 tiles side by side: a left move makes a 65,536 tile


def start_boards(n: int, reset_boards: np.ndarray, seed: int) -> np.ndarray:
    """Start boards by lane index mod 4: the reset board itself; random ~60 % filled; full random (many end within
    a few moves); full with no legal move (odd exponents on one checkerboard colour, even on the other).
    Exponents 1..11."""
    g = np.random.default_rng(seed)
    e = g.integers(1, 12, size=(n, 16))
    sparse = (np.arange(n) % 4 == 1)[:, None] & (g.random((n, 16)) >= 0.6)
    e[sparse] = 0
    colour = (np.arange(16) // 4 + np.arange(16) % 4) % 2
    stuck = 1 + colour[None, :] + 2 * g.integers(0, 5, size=(n, 16))
    e = np.where((np.arange(n) % 4 == 3)[:, None], stuck, e).astype(np.uint64)
    packed = (e << (4 * np.arange(16, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)
    return np.where(np.arange(n) % 4 == 0, reset_boards, packed)


class LaneRef:
    """One O.Env with the device's lane bookkeeping restated in Python."""

    def __init__(self, rng, auto_reset, cfg):
        self.env = O.Env(rng=rng, philox_key=KEY, **cfg)
        self.auto_reset, self.active = auto_reset, False

    def reset(self, seed):
        self.env.reset(seed)
        self.active = True

    def set_board(self, packed):
        ex = O.unpack_exponents(int(packed)).reshape(16)
        for c in range(16):
            self.env.e.game.board[c] = (1 << int(ex[c])) if ex[c] else 0
        self.env.e.step_count, self.env.e.game.step_count, self.env.e.max_tile_seen = 0, 0, 4

    def packed(self):
        out = ctypes.c_uint64()
        rc = O.lib().or_pack_board(self.env.e.game.board, ctypes.byref(out))
        return (0, 1) if rc else (int(out.value), 0)

    def step(self, action):
        e = self.env
        o = dict(reward=0.0, flags=0, prev_board=self.packed()[0], score_add=0, merged=[0] * 8, n_merged=0)
        if not self.active:
            o["flags"] = O.B_INACTIVE
        elif action > 3:
            o["flags"] = O.B_BADACTION
        else:
            score0 = e.score
            r = e.step(int(action))
            nm = int(e.e.game.n_merged)
            o.update(reward=r["reward"], score_add=e.score - score0, n_merged=nm,
                     merged=[int(e.e.game.merged[k]) if k < nm else 0 for k in range(8)],
                     flags=(O.B_CHANGED * r["changed"] | O.B_TERMINATED * r["terminated"]
                            | O.B_TRUNCATED * r["truncated"] | O.B_INVALID * r["invalid"]))
            if r["terminated"] or r["truncated"]:
                if self.auto_reset:
                    o["flags"] |= O.B_RESET
                    e.reset((e.seed + STRIDE) & 0xFFFFFFFFFFFFFFFF)
                else:
                    self.active = False
        return o

    def state(self):
        e = self.env
        n = 272 if e.cfg.obs_mode == 2 else 16
        obs = (ctypes.c_float * n)()
        O.lib().or_env_obs(ctypes.byref(e.e), ctypes.byref(e.cfg), obs)   # -1 (a 65,536 tile) leaves a partial row
        board, unrep = self.packed()
        g = e.e.game.rng
        return dict(board=board, unrepresentable=unrep, mask=int((e.mask() * (1, 2, 4, 8)).sum()),
                    obs=np.array(obs[:], dtype=np.float32), score=e.score, step_count=e.step_count,
                    max_tile_seen=e.max_tile_seen, seed=e.seed, active=int(self.active),
                    rng_state=[g.state_lo, g.state_hi], rng_inc=[g.inc_lo, g.inc_hi], has_uint32=g.has_uint32,
                    uinteger=g.uinteger)


def assert_lanes_equal(got: dict, lanes: list, tag):
    """Every output array of the batch == the per-lane values, bit for bit (floats compared as their bits)."""
    for k, arr in got.items():
        want = np.array([d[k] for d in lanes], dtype=arr.dtype).reshape(arr.shape)
        bits = {4: np.uint32, 8: np.uint64}[arr.itemsize] if arr.dtype.kind == "f" else arr.dtype
        bad = np.nonzero((arr.view(bits) != want.view(bits)).reshape(len(lanes), -1).any(axis=1))[0]
        assert bad.size == 0, (tag, k, int(bad[0]), arr[bad[0]], want[bad[0]])


def with_truncation(cfg):
    """ENV_CFGS entries that leave max_steps at 1,024 get a limit this run can reach."""
    return dict(cfg, max_steps=cfg["max_steps"] if "max_steps" in cfg else 25)


def setup(batch, refs, seeds):
    n = batch.n
    st = batch.reset(seeds)
    boards = start_boards(n, st["board"].copy(), seed=77)
    boards[UNREP_LANE] = 0xFF          # row 0: 2**15, 2**15, 0, 0
    for e, s in zip(refs, seeds):
        e.reset(int(s))
    for e, b in zip(refs, boards):
        e.set_board(b)
    return batch.set_boards(boards)


@pytest.mark.parametrize("auto_reset", [False, True], ids=["once", "autoreset"])
@pytest.mark.parametrize("rng", ["pcg64", "philox"])
@pytest.mark.parametrize("ci", range(len(ENV_CFGS)))
def test_env_batch_equals_per_lane_env(ci, rng, auto_reset):
    cfg = with_truncation(ENV_CFGS[ci])
    batch = O.EnvBatch(N, rng=rng, philox_key=KEY, auto_reset=auto_reset, reset_stride=STRIDE, **cfg)
    refs = [LaneRef(rng, auto_reset, cfg) for _ in range(N)]
    seeds = np.arange(N, dtype=np.uint64) * 13 + 7000
    st = setup(batch, refs, seeds)
    assert_lanes_equal(st, [e.state() for e in refs], "start")
    g = np.random.default_rng(5)
    seen = dict(term=0, trunc=0, invalid=0, reset=0, inactive=0, bad=0, unrep=0)
    for t in range(T):
        acts = g.integers(0, 4, size=N).astype(np.uint8)
        acts[UNREP_LANE] = 3
        wild = g.random(N) < 0.03
        acts[wild] = g.integers(4, 256, size=int(wild.sum()))
        got = batch.step(acts)
        want = [{**e.step(int(a)), **e.state()} for e, a in zip(refs, acts)]
        assert_lanes_equal(got, want, t)
        fl = got["flags"]
        assert batch.stepped == int(((fl & (O.B_INACTIVE | O.B_BADACTION)) == 0).sum())
        for k, bit in (("term", O.B_TERMINATED), ("trunc", O.B_TRUNCATED), ("invalid", O.B_INVALID),
                       ("reset", O.B_RESET), ("inactive", O.B_INACTIVE), ("bad", O.B_BADACTION)):
            seen[k] += int(((fl & bit) != 0).sum())
        seen["unrep"] += int(got["unrepresentable"].sum())
    assert seen["term"] > 0 and seen["trunc"] > 0 and seen["invalid"] > 0 and seen["bad"] > 0, seen
    assert (seen["reset"] > N and seen["inactive"] == 0) if auto_reset else (seen["reset"] == 0 and seen["inactive"] > N)
    if not (auto_reset and cfg["max_steps"] == 0):   # there the 65,536 lane restarts in the step that makes the tile
        assert seen["unrep"] > 0, seen


def test_partial_reset_and_partial_board_set():
    """reset / set_boards under a lane mask touch the chosen lanes only."""
    cfg = with_truncation(ENV_CFGS[2])
    batch = O.EnvBatch(N, auto_reset=True, reset_stride=STRIDE, **cfg)
    refs = [LaneRef("pcg64", True, cfg) for _ in range(N)]
    setup(batch, refs, np.arange(N, dtype=np.uint64) + 50)
    g = np.random.default_rng(8)
    for t in range(6):
        acts = g.integers(0, 4, size=N).astype(np.uint8)
        batch.step(acts)
        for e, a in zip(refs, acts):
            e.step(int(a))
    sel = g.random(N) < 0.5
    seeds = np.arange(N, dtype=np.uint64) + 90_000
    st = batch.reset(seeds, mask=sel)
    for i in np.nonzero(sel)[0]:
        refs[i].reset(int(seeds[i]))
    assert_lanes_equal(st, [e.state() for e in refs], "partial reset")
    sel2 = g.random(N) < 0.5
    boards = start_boards(N, st["board"].copy(), seed=3)
    st = batch.set_boards(boards, mask=sel2)
    for i in np.nonzero(sel2)[0]:
        refs[i].set_board(boards[i])
    assert_lanes_equal(st, [e.state() for e in refs], "partial set")


def run_digest(n=4096, steps=20) -> str:
    """sha256 over every output of a fixed run (both RNGs, auto-reset on and off)."""
    h = hashlib.sha256()
    cfg = with_truncation(ENV_CFGS[2])
    for rng in ("pcg64", "philox"):
        for auto_reset in (False, True):
            batch = O.EnvBatch(n, rng=rng, philox_key=KEY, auto_reset=auto_reset, reset_stride=n, **cfg)
            st = batch.reset(np.arange(n, dtype=np.uint64) + 31)
            batch.set_boards(start_boards(n, st["board"].copy(), seed=9))
            g = np.random.default_rng(2)
            for t in range(steps):
                out = batch.step(g.integers(0, 5, size=n).astype(np.uint8))
                for k in sorted(out):
                    h.update(out[k].tobytes())
    return h.hexdigest()


def test_same_bits_for_one_thread_and_the_default():
    """Lanes are independent, so the OpenMP loops give the same outputs for OMP_NUM_THREADS=1 (a fresh process:
    the runtime reads the variable when it loads) and for the default thread count of this process."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_oracle_batch as t\n"
            "print(t.O.batch_max_threads(), t.run_digest())\n" % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, check=True)
    threads, digest = r.stdout.split()[-2:]
    assert int(threads) == 1
    assert digest == run_digest(), (threads, O.batch_max_threads())


def test_missing_symbols_point_at_build(monkeypatch):
    """A liboracle.so from before the batched entry points is reported as such, with the way to rebuild it."""
    class Old:
        pass

    monkeypatch.setattr(O, "_batch_ready", False)
    monkeypatch.setattr(O, "lib", lambda: Old())
    with pytest.raises(RuntimeError, match=r"older build without or_batch_reset.*build\(\)"):
        O.EnvBatch(4)
