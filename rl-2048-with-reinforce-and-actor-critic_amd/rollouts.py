"""Host driver of the persistent rollout and evaluation launches (g2048_rollout, g2048_deep_rollout,
g2048_sized_rollout, g2048_scripted_* and their score-only *_eval forms): the per-episode buffers and the launch ->
read the suspended count -> resume loops every family shares.  What differs between families is one C call, handed in
as ``launch(order, n_order, resume, sus, limit)``; nothing here knows an agent, and nothing needs a device except
the tensors it is told to allocate there (tests/test_rollout_driver_cpu.py runs the loops on CPU tensors)."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L


def seed_seq(seeds):
    """A batch of episode seeds as a tensor / numpy array (kept: the fast conversion path) or a list."""
    return seeds if isinstance(seeds, (torch.Tensor, np.ndarray)) else list(seeds)


def pcg64_stream(lib, seeds: torch.Tensor, stream, seeded: bool = True):
    """(state [2n], increment [2n], buffered uint32 [n]) of one PCG64 stream per uint64 seed, seeded like
    numpy.random.default_rng(seed) by g2048_seed_pcg64 (seeded=False: allocated only)."""
    n, dev = seeds.numel(), seeds.device
    st = torch.empty(2 * n, dtype=torch.int64, device=dev)
    inc = torch.empty(2 * n, dtype=torch.int64, device=dev)
    buf = torch.empty(n, dtype=torch.int64, device=dev)
    if seeded:
        L.check(lib.g2048_seed_pcg64(L.ptr(seeds), L.ptr(st), L.ptr(inc), L.ptr(buf), n, stream))
    return st, inc, buf


def episode_streams(lib, env_seeds, policy_seeds, device, stream):
    """The two PCG64 streams of every episode as the kernels take them -- env state, increment, buffer, then the
    policy's three -- and the two uint64 seed tensors they were made from.  The caller keeps the seeds until its call
    ends: freed here, their blocks would go to the per-episode outputs that outlive the call."""
    from .vec_env import _as_u64_seeds

    n = len(env_seeds)
    es = _as_u64_seeds(seed_seq(env_seeds), n, 0, device)
    ps = _as_u64_seeds(seed_seq(policy_seeds), n, 0, device)
    return [*pcg64_stream(lib, es, stream), *pcg64_stream(lib, ps, stream)], (es, ps)


def _boards(W, n: int, device, rows: int | None = None) -> torch.Tensor:
    """Uninitialised boards of n episodes (rows: per time row): bitboards, or W planes for sizes other than 4."""
    shape = (n,) if rows is None else (rows, n)
    return torch.empty(shape if W is None else (W,) + shape, dtype=torch.int64, device=device)


# The classes below hand the kernels data_ptr() of tensors they have just allocated (or concatenated), which are
# contiguous by construction: L.ptr's check is for buffers that come from elsewhere.

class EpisodeOutputs:
    """What a persistent kernel writes once per episode: lengths, totals, the largest tile's exponent and the final
    board ([n], or [W, n] planes)."""

    def __init__(self, n: int, device, W: int | None = None):
        self.n = n
        self.lengths = torch.empty(n, dtype=torch.int32, device=device)
        self.totals = torch.empty(n, dtype=torch.float64, device=device)
        self.max_e = torch.empty(n, dtype=torch.uint8, device=device)
        self.final = _boards(W, n, device)
        # the fields of L.EvalOut, which are the last four of L.Traj
        self.pointers = (self.lengths.data_ptr(), self.totals.data_ptr(), self.max_e.data_ptr(), self.final.data_ptr())

    def eval_out(self) -> L.EvalOut:
        return L.EvalOut(*self.pointers)

    @property
    def max_tile(self) -> torch.Tensor:
        return 1 << self.max_e.to(torch.int64)

    def longest(self) -> int:
        """The longest episode's steps (one host sync)."""
        return int(self.lengths.max().item()) if self.n else 0


class TrajectoryRows:
    """The time-major rows of a batch, [cap, n] ([W, cap, n] board planes for sizes other than 4), pre-filled with
    what a row past an episode's end holds: action 0, reward 0.0, flags F_INACTIVE, probabilities 0 (boards are left
    uninitialised).  Starts with `cap` rows, the first capacity; grow() adds more and keeps what was written."""

    def __init__(self, n: int, device, W: int | None = None, probs: bool = False, cap: int = 0):
        self.n, self.device, self.W, self.cap = n, device, W, 0
        self.row_bytes = n * (8 * (W or 1) + 1 + 8 + 1 + (16 if probs else 0))
        self.boards = self.actions = self.rewards = self.flags = self.probs = None
        self._probs = probs
        if cap:
            self.grow(cap)

    def grow(self, rows: int) -> None:
        n, dev = self.n, self.device
        boards = _boards(self.W, n, dev, rows)
        actions = torch.zeros(rows, n, dtype=torch.uint8, device=dev)
        rewards = torch.zeros(rows, n, dtype=torch.float64, device=dev)
        flags = torch.full((rows, n), L.F_INACTIVE, dtype=torch.uint8, device=dev)
        probs = torch.zeros(rows, n, 4, dtype=torch.float32, device=dev) if self._probs else None
        if self.cap:
            boards = torch.cat([self.boards, boards], dim=0 if self.W is None else 1)    # planes: along their rows
            actions = torch.cat([self.actions, actions])
            rewards = torch.cat([self.rewards, rewards])
            flags = torch.cat([self.flags, flags])
            if probs is not None:
                probs = torch.cat([self.probs, probs])
        self.boards, self.actions, self.rewards, self.flags, self.probs = boards, actions, rewards, flags, probs
        self.cap += rows

    @property
    def plane_stride(self) -> int:
        """Elements between two board planes (the sized kernels' argument)."""
        return self.cap * self.n

    def pointers(self) -> tuple:
        """The first five fields of L.Traj (probs NULL unless recorded)."""
        return (self.boards.data_ptr(), self.actions.data_ptr(), self.rewards.data_ptr(), self.flags.data_ptr(),
                None if self.probs is None else self.probs.data_ptr())

    def traj(self, outs: EpisodeOutputs) -> L.Traj:
        return L.Traj(*self.pointers(), *outs.pointers)

    def sliced(self, T: int) -> dict:
        """The first T rows of every field, by name."""
        return {"boards": self.boards[:T] if self.W is None else self.boards[:, :T], "actions": self.actions[:T],
                "rewards": self.rewards[:T], "flags": self.flags[:T],
                "probs": None if self.probs is None else self.probs[:T]}


class SuspendState:
    """Where a persistent kernel parks the episodes that reached a launch's row / step limit: board, step count and
    stream positions (meta), running total, and the list of their ids with its count.  Two lists (the second made when
    a launch first suspends): a resume launch reads its order from the one the previous launch filled while it fills
    the other."""

    def __init__(self, n: int, device, W: int | None = None):
        self.board = _boards(W, n, device)
        self.meta = torch.empty(3 * n, dtype=torch.int32, device=device)
        self.total = torch.empty(n, dtype=torch.float64, device=device)
        self.list = torch.empty(max(n, 1), dtype=torch.int32, device=device)     # the one the next launch fills
        self.count = torch.zeros(1, dtype=torch.int32, device=device)
        self._other = None                                                       # made when a launch first suspends

    def struct(self) -> L.Suspend:
        return L.Suspend(self.board.data_ptr(), self.meta.data_ptr(), self.total.data_ptr(), self.list.data_ptr(),
                         self.count.data_ptr())

    def suspended(self) -> int:
        """Episodes the last launch suspended (one host sync)."""
        return int(self.count.item())

    def flip(self) -> torch.Tensor:
        """The list just filled, as the next launch's order; that launch fills the other list from a zero count."""
        order = self.list
        self.list = torch.empty_like(order) if self._other is None else self._other
        self._other = order
        self.count.zero_()
        return order


def run_growing(launch, rows: TrajectoryRows, outs: EpisodeOutputs, sus: SuspendState | None, queue: torch.Tensor,
                n: int, max_steps: int | None, max_rows: int, free_bytes, hint: str) -> int:
    """Play n episodes into trajectory rows (which come with their first capacity): launch(order, n_order, resume, sus,
    cap) runs every episode until it ends or fills the `cap` rows; the kernel suspends those that filled them, the rows
    grow (x2, never past max_steps) and one more launch resumes just those.  sus None: the kernel bounds its episodes
    itself -- one launch, no count read.  Returns T, the longest episode's steps.

    The batch is time-major [T, n] for all n episodes (the update's layout), so a few long episodes grow every lane's
    rows.  An episode that never ends (max_steps None with invalid actions allowed, where the reference itself would
    loop forever) must not run the device out of memory: refuse past the rows the free memory holds (free_bytes():
    free device memory plus what the caching allocator holds reserved but unused, which torch.cat reuses or releases
    before it would fail), or past max_rows."""
    order, n_order, resume = None, n, 0
    while True:
        launch(order, n_order, resume, sus, rows.cap)
        k = sus.suspended() if sus is not None else 0
        if k == 0:
            return outs.longest()
        order, n_order, resume = sus.flip(), k, 1
        queue.zero_()
        cap, row_bytes = rows.cap, rows.row_bytes
        grow = cap if max_steps is None else max(min(cap, int(max_steps) - cap), 1)
        free_b = free_bytes()
        if cap + grow > max_rows or (cap + grow) * row_bytes > free_b + cap * row_bytes // 2:
            raise RuntimeError(
                f"rollout_batch (max_steps=None): {k} episode(s) still running after {cap} steps; growing the "
                f"[T, n] trajectory buffer to {cap + grow} rows needs {(cap + grow) * row_bytes / 2**30:.1f} GiB "
                f"(free: {free_b / 2**30:.1f} GiB, row limit {max_rows}) -- {hint}")
        rows.grow(grow)


def run_budgeted(launch, sus: SuspendState | None, queue: torch.Tensor, n: int, budget: int, most: int,
                 hint: str) -> None:
    """Play n episodes for their scores alone: launch(order, n_order, resume, sus, limit) may take every episode to
    `limit` steps in all before the kernel suspends it (so every launch is bounded); the suspended ones are relaunched
    with `budget` more steps, and refused once they would pass `most` (an episode that never ends raises instead of
    being relaunched for ever).  Nothing grows between launches.  sus None: one launch, as run_growing."""
    limit = min(budget, most)
    order, n_order, resume = None, n, 0
    while True:
        launch(order, n_order, resume, sus, limit)
        k = sus.suspended() if sus is not None else 0
        if k == 0:
            return
        if limit >= most:
            raise RuntimeError(
                f"evaluate_batch: {k} episode(s) still running after {limit} steps; playing on would pass "
                f"eval_max_steps = {most} -- {hint}")
        order, n_order, resume = sus.flip(), k, 1
        queue.zero_()
        limit = min(limit + budget, most)
