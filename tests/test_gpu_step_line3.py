"""Every lane of the log2-reward step kernel (step_kernel<..., RK = 1>: the three-cell line table, 16 KiB, and a
reset list of its own in LDS) against the batched CPU oracle (oracle.EnvBatch), the way tests/test_gpu_step_matrix.py
compares: every output and every lane-state word after every step, equality only.

* test_crafted_lines: n = 16,384 + 37 (the smallest batch that stages the table in LDS, with a ragged tail) and
  n = 16,383 (the table read through L1), 6 steps, all four actions in every wave.  Three boards in four carry a
  crafted line in a random slot, as a row or a column, forwards or backwards: empty, full, [a,a,a,a], [0,a,a,a],
  [a,a,b,b], [a,b,b,a], 14+14 and 15+15 pairs.  A lane whose move merges 2**15 + 2**15 (the oracle's merged list
  holds 65536) must raise the overflow flag, and only such a lane may; it is compared on that step's changed flag and
  reward, then dropped, because its nibble board holds 2**15 where the reference holds 65536.
* test_every_lane_resets_in_one_step: max_steps = 1 with auto-reset at n = 16,384 + 37, so every lane of every wave
  goes through the workgroup's reset list in the same launch.  A workgroup's list holds four entries per thread and at
  this size each wave runs one sweep: the dense pass takes them all.
* test_reset_list_overflow: the same at 5 sweeps per wave (5 x 1024 x CUs + 37 lanes): every workgroup collects more
  resets than its list holds, so the lanes past the end do their own reset (the full-list fallback).
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_step_matrix import DEV, KEY, K_BLOCK, K_LUT_SMALL_N, N, Case, _eq, _u64, env_cfg

pytestmark = pytest.mark.gpu
K_RESET_ENTRIES_PER_THREAD = 4     # csrc/g2048.hip Step3Lds::kCap = 4 * threads of the workgroup

LINES = ([0, 0, 0, 0], [1, 2, 3, 4], [7, 5, 7, 5], [3, 3, 3, 3], [0, 6, 6, 6], [2, 2, 9, 9], [4, 8, 8, 4], [5, 5, 0, 5],
         [0, 0, 0, 11], [14, 14, 0, 0], [13, 14, 14, 0], [15, 15, 0, 0], [0, 15, 15, 15], [15, 15, 15, 15],
         [14, 14, 15, 15], [15, 0, 15, 3], [3, 15, 0, 15], [15, 15, 14, 14])


def crafted_boards(n, reset_boards, seed):
    """Lane i % 4 == 0 keeps its reset board; the others are random (exponents 0..12, ~30 % empty) with one of LINES
    written over a random row or column, forwards or backwards."""
    g = np.random.default_rng(seed)
    e = g.integers(1, 13, size=(n, 4, 4))
    e[g.random((n, 4, 4)) < 0.3] = 0
    which, slot = g.integers(0, len(LINES), size=n), g.integers(0, 4, size=n)
    col, rev = g.integers(0, 2, size=n).astype(bool), g.integers(0, 2, size=n).astype(bool)
    lines = np.array(LINES)[which]
    lines = np.where(rev[:, None], lines[:, ::-1], lines)
    idx = np.arange(n)
    rows = e.copy()
    rows[idx, slot, :] = lines
    cols = e.copy()
    cols[idx, :, slot] = lines
    e = np.where(col[:, None, None], cols, rows).reshape(n, 16).astype(np.uint64)
    packed = (e << (4 * np.arange(16, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)
    return np.where(idx % 4 == 0, reset_boards, packed)


class LineCase:
    """One VecGame2048Env on crafted boards and its EnvBatch twin, compared lane for lane while the lane is live."""

    def __init__(self, n, obs, rng, packed, case):
        from rl2048_amd import Game2048EnvConfig, VecGame2048Env
        from rl2048_amd import _lib as L

        self.L, self.n, self.pcg, self.packed = L, n, rng == "pcg64", packed
        cfg = dict(env_cfg(case, obs, "log2"), max_steps=5)
        self.env = env = VecGame2048Env(n, Game2048EnvConfig(**cfg), device=DEV, rng=rng, auto_reset=True,
                                        reset_stride=n, philox_key=KEY, track_score=False, packed_mask=packed)
        want = ["reward", "flags", "merged", "board", "unrepresentable", "mask", "obs", "step_count", "max_tile_seen",
                "seed", "active"] + (["rng_state", "rng_inc", "has_uint32", "uinteger"] if self.pcg else [])
        self.ref = O.EnvBatch(n, rng=rng, philox_key=KEY, auto_reset=True, reset_stride=n, outputs=want, **cfg)
        seeds = np.arange(n, dtype=np.uint64) * 5 + 77_000
        env.reset(seed=torch.from_numpy(seeds.view(np.int64)).to(DEV))
        st = self.ref.reset(seeds)
        b = crafted_boards(n, st["board"].copy(), seed=99 + case)
        env.board.copy_(torch.from_numpy(b.view(np.int64)).to(DEV))
        self.ref.set_boards(b)
        self.live = np.ones(n, dtype=bool)
        self.g = np.random.default_rng(31 + case)
        self.count = dict(sat=0, m15=0, term=0, trunc=0, invalid=0, reset=0)

    def step(self, t):
        env, L, n = self.env, self.L, self.n
        acts = self.g.integers(0, 4, size=n).astype(np.uint8)
        acts[(np.arange(n) % 64) < 4] = np.arange(n)[(np.arange(n) % 64) < 4] % 4     # all four actions in every wave
        env.step_into(torch.from_numpy(acts).to(DEV))
        ref = self.ref.step(acts)
        fl, rfl = env.flags.cpu().numpy(), ref["flags"]
        sat = (ref["merged"] == 65536).any(axis=1) & self.live
        was, ok = np.nonzero(self.live)[0], np.nonzero(self.live & ~sat)[0]
        _eq("overflow flag", (fl[was] & L.F_OVERFLOW) != 0, sat[was], t, lanes=was)
        rw, rrw = env.reward.cpu().numpy(), ref["reward"].astype(np.float32)
        # a saturating step: changed, and the reward unless the episode's end differs (the nibble board may keep two
        # mergeable 2**15 tiles where the reference's 65536 cannot merge: DESIGN.md section 7)
        s = np.nonzero(sat)[0]
        _eq("changed (saturated)", fl[s] & L.F_CHANGED, rfl[s] & O.B_CHANGED, t, lanes=s)
        same_end = s[(fl[s] & L.F_TERMINATED) == (rfl[s] & O.B_TERMINATED)]
        _eq("reward (saturated)", rw[same_end], rrw[same_end], t, lanes=same_end)
        self.live &= ~sat
        # every other live lane: everything
        _eq("flags", fl[ok], rfl[ok], t, lanes=ok)
        _eq("reward", rw[ok], rrw[ok], t, lanes=ok)
        assert int(ref["unrepresentable"][ok].sum()) == 0, t
        _eq("board", _u64(env.board)[ok], ref["board"][ok], t, lanes=ok)
        _eq("seed", _u64(env.seed)[ok], ref["seed"][ok], t, lanes=ok)
        has = ref["has_uint32"].astype(bool) if self.pcg else np.zeros(n, dtype=bool)
        word = (ref["step_count"].astype(np.uint32)
                | (np.log2(np.maximum(ref["max_tile_seen"], 1)).astype(np.uint32) << L.LS_MAXT_SHIFT)
                | np.where(ref["active"] != 0, L.LS_ACTIVE, 0).astype(np.uint32)
                | np.where(has, L.LS_HAS_U32, 0).astype(np.uint32))
        _eq("state word", env.state.cpu().numpy().view(np.uint32)[ok], word[ok], t, lanes=ok)
        if self.pcg:
            _eq("rng_state", _u64(env.rng_state).reshape(n, 2)[ok], ref["rng_state"][ok], t, lanes=ok)
            _eq("rng_inc", _u64(env.rng_inc).reshape(n, 2)[ok], ref["rng_inc"][ok], t, lanes=ok)
            hu = ok[has[ok]]
            _eq("rng_uint", env.rng_uint.cpu().numpy().view(np.uint32)[hu], ref["uinteger"][hu], t, lanes=hu)
        if self.packed:
            _eq("mask_bits", env.mask_bits.cpu().numpy()[ok], ref["mask"][ok], t, lanes=ok)
        else:
            bits = ((ref["mask"][:, None] >> np.arange(4)) & 1).astype(np.int8)
            _eq("mask", env.mask.cpu().numpy()[ok], bits[ok], t, lanes=ok)
        _eq("obs", env.obs.cpu().numpy()[ok], ref["obs"][ok], t, lanes=ok)
        c = self.count
        c["sat"] += int(sat.sum())
        c["m15"] += int((ref["merged"][ok] == 32768).any(axis=1).sum())
        c["term"] += int(((rfl[ok] & O.B_TERMINATED) != 0).sum())
        c["trunc"] += int(((rfl[ok] & O.B_TRUNCATED) != 0).sum())
        c["invalid"] += int(((rfl[ok] & O.B_INVALID) != 0).sum())
        c["reset"] += int(((rfl[ok] & O.B_RESET) != 0).sum())


CRAFTED = [(N, "log2", "pcg64", True), (N, "onehot", "philox", False), (K_LUT_SMALL_N - 1, "log2", "pcg64", True)]


@pytest.mark.parametrize("n,obs,rng,packed", CRAFTED,
                         ids=[f"n{n}-{o}-{r}-{'packed' if p else 'int8'}" for n, o, r, p in CRAFTED])
def test_crafted_lines(n, obs, rng, packed):
    c = LineCase(n, obs, rng, packed, case=0)       # case 0 of env_cfg: log2 rewards, raw bonus, masked
    for t in range(6):
        c.step(t)
    k = c.count
    assert k["sat"] > 100 and k["m15"] > 100, k      # 15+15 (the per-line fallback) and 14+14 merges happened
    assert k["trunc"] > 0 and k["invalid"] > 0 and k["reset"] > n // 2, k
    assert int(c.live.sum()) > n // 2, k


def test_every_lane_resets_in_one_step():
    """max_steps = 1: each step truncates (or ends) every lane, and every lane is reset through the LDS list."""
    assert N <= K_RESET_ENTRIES_PER_THREAD * K_BLOCK * -(-N // K_BLOCK)     # no list overflows here
    c = Case(N, "log2", "pcg64", "xo3_rk1", case=0, max_steps=1)
    for _ in range(3):
        fl = c.step()
        assert bool(((fl & O.B_RESET) != 0).all())
    assert c.count["term"] > 0 and c.count["trunc"] > N, c.count


def test_reset_list_overflow():
    """5 sweeps per wave, every lane resetting: each workgroup's list (4 entries per thread) overflows."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sweeps = K_RESET_ENTRIES_PER_THREAD + 1
    n = sweeps * K_BLOCK * cus + 37
    c = Case(n, "log2", "pcg64", "xo3_rk1", case=0, max_steps=1, boards="reset")
    for _ in range(2):
        fl = c.step()
        both = O.B_RESET | O.B_TRUNCATED             # a fresh game cannot end within one move
        assert bool(((fl & both) == both).all())
    assert int(c.resets.min()) == 2 == int(c.resets.max())
