"""An n-tuple value network for 2048 and the players that read it (include/g2048_ntuple.h): NTupleNetwork holds the
int32 fixed-point weights on the device, NTuplePolicy is the ``action_gen`` that rollout_batch / evaluate_batch /
run_episode / evaluation_loop play on the device, and ReinforceAgent.ntuple_update trains the weights by afterstate
TD(0) on a recorded TrajectoryBatch.  Everything is integer arithmetic, so this module's pure-Python statement of the
model, the host build of csrc/g2048_ntuple_core.h and the device kernels agree bit for bit.

The model.  A board is N x N exponents e[cell], cell = r N + c, 0 = empty; move(b, a) is the env's slide / merge without
the spawn, a is valid iff move(b, a) != b, g(b, a) is the sum of the merged tiles' values (0 for an invalid move).

  F = 10 fractional bits (FRAC_BITS): a reward in value units is g << F
  B base tuples (1 <= B <= 16), tuple t = k_t distinct cells (2 <= k_t <= 6) with its own table of 16^k_t int32
  weights; all tables lie in one buffer, table t at offset sum_{s<t} 16^k_s
  features: the 8 dihedral images of every base tuple -- (r, c), (c, N-1-r), (N-1-r, N-1-c), (N-1-c, r) and the
  transposes of those four -- each sharing its base tuple's table: 8 B features.  Images that coincide stay separate
  features and count twice.
  index_f(m) = sum_j e[cells_f[j]] 16^j;   V(m) = sum_f w[offset_f + index_f(m)]
  Q_0(b, a)  = (g(b, a) << F) + V(move(b, a))                         for valid a
  V'(s)      = max over valid a' of Q_0(s, a'), 0 when none is valid
  Q_1(b, a)  = (g << F) + (sum over empty c of m of 9 V'(m + a 2 at c) + V'(m + a 4 at c)) // (10 #empty(m)),
               m = move(b, a); // is Python's floor division
  choice     = the valid action of the largest Q_depth, the lowest index among equals; 0 when none is valid
"""
from __future__ import annotations

import ctypes
import operator

import numpy as np
import torch

from . import _lib as L

FRAC_BITS = L.NTUPLE_FRAC_BITS
INVALID_Q = -(1 << 63)
MAX_BASE_TUPLES = 16
_M64 = (1 << 64) - 1


def hash_weights(table: int, count: int, seed: int) -> np.ndarray:
    """The weights fill_hash gives table `table` (its first `count` entries), int32 in -32768..32767:

        x = (seed * 0x9E3779B97F4A7C15 + table * 0xBF58476D1CE4E5B9 + index * 0x94D049BB133111EB + 1) mod 2^64
        x ^= x >> 31;  x = x * 0xD6E8FEB86659FD93 mod 2^64;  x ^= x >> 29
        w = (x >> 48) - 32768
    """
    base = (int(seed) * 0x9E3779B97F4A7C15 + int(table) * 0xBF58476D1CE4E5B9 + 1) & _M64
    with np.errstate(over="ignore"):
        x = np.arange(count, dtype=np.uint64) * np.uint64(0x94D049BB133111EB) + np.uint64(base)
        x ^= x >> np.uint64(31)
        x *= np.uint64(0xD6E8FEB86659FD93)
        x ^= x >> np.uint64(29)
    return ((x >> np.uint64(48)).astype(np.int64) - 32768).astype(np.int32)


def dihedral_images(cells, n: int) -> list:
    """The 8 images of a tuple of cells on an n x n board, in the order of the module docstring."""
    maps = [lambda r, c: (r, c), lambda r, c: (c, n - 1 - r), lambda r, c: (n - 1 - r, n - 1 - c),
            lambda r, c: (n - 1 - c, r)]
    out = []
    for transpose in (False, True):
        for f in maps:
            img = []
            for cell in cells:
                r, c = f(cell // n, cell % n)
                if transpose:
                    r, c = c, r
                img.append(r * n + c)
            out.append(tuple(img))
    return out


def _slide_score(line):
    """One line moved towards its first cell (exponents, 0 = empty): (new line, sum of the merged tiles' values).  As
    on the device's nibble board, a 2^15 + 2^15 merge leaves 2^15 on the board; its gain is the true 65536."""
    tiles = [e for e in line if e]
    out, score, i = [], 0, 0
    while i < len(tiles):
        if i + 1 < len(tiles) and tiles[i] == tiles[i + 1]:
            out.append(min(tiles[i] + 1, 15))
            score += 1 << (tiles[i] + 1)
            i += 2
        else:
            out.append(tiles[i])
            i += 1
    return out + [0] * (len(line) - len(out)), score


def move_score(b, n: int, a: int):
    """move(b, a) without the spawn on a row-major tuple of n x n exponents: (new board, g(b, a))."""
    nb, score = list(b), 0
    for k in range(n):
        idx = [k * n + j for j in range(n)] if a in (1, 3) else [j * n + k for j in range(n)]
        if a in (1, 2):
            idx.reverse()
        new, g = _slide_score([b[i] for i in idx])
        score += g
        for i, v in zip(idx, new):
            nb[i] = v
    return tuple(nb), score


class NTupleNetwork:
    """The weights and feature list of an n-tuple network on boards of `size` x `size` cells (module docstring).

    tuples: the base tuples, each a sequence of 2..6 distinct cell indices (default: default_tuples(size)).  weights: one
    int32 tensor on `device`, zero-initialised, holding every table; train it with ReinforceAgent.ntuple_update, set it
    with fill_hash / load_state_dict.  features: [(table, offset, cells)] for the 8 images of every base tuple, the flat
    list the device reads."""

    def __init__(self, size: int, tuples=None, device="cuda"):
        try:
            size = operator.index(size)
        except TypeError:
            raise ValueError(f"size must be an integer in 2..8, got {size!r}") from None
        if not 2 <= size <= 8:
            raise ValueError(f"size must be an integer in 2..8, got {size!r}")
        self.size = size
        base = self.default_tuples(size) if tuples is None else [tuple(operator.index(c) for c in t) for t in tuples]
        if not 1 <= len(base) <= MAX_BASE_TUPLES:
            raise ValueError(f"an n-tuple network has 1..{MAX_BASE_TUPLES} base tuples (got {len(base)})")
        for t in base:
            if not L.NTUPLE_MIN_CELLS <= len(t) <= L.NTUPLE_MAX_CELLS:
                raise ValueError(f"a tuple has {L.NTUPLE_MIN_CELLS}..{L.NTUPLE_MAX_CELLS} cells (got {t!r})")
            if len(set(t)) != len(t) or min(t) < 0 or max(t) >= size * size:
                raise ValueError(f"a tuple's cells are distinct and in 0..{size * size - 1} (got {t!r})")
        self.tuples = base
        self.offsets, off = [], 0
        for t in base:
            self.offsets.append(off)
            off += 16 ** len(t)
        self.n_weights = off
        self.features = [(ti, self.offsets[ti], img) for ti, t in enumerate(base) for img in dihedral_images(t, size)]
        self.device = torch.device(device)
        self.weights = torch.zeros(self.n_weights, dtype=torch.int32, device=self.device)
        self._host = None            # a numpy copy of the weights for the pure-Python statement; dropped on any write
        self._feat = (L.NTupleFeature * len(self.features))(*[
            L.NTupleFeature(o, len(c), (ctypes.c_uint8 * 6)(*c), 0) for _, o, c in self.features])

    @staticmethod
    def default_tuples(size: int) -> list:
        """With h = ceil(size / 2) and k = min(size, 4): the horizontal runs of k cells starting at column 0 of rows
        0..h-1, then the 2 x 2 squares with top-left (r, c), 0 <= r <= c < h.  size 4 gives the classic five: outer
        row, inner row, corner, edge and centre square."""
        h, k = (size + 1) // 2, min(size, 4)
        rows = [tuple(r * size + j for j in range(k)) for r in range(h)]
        squares = [(r * size + c, r * size + c + 1, (r + 1) * size + c, (r + 1) * size + c + 1)
                   for r in range(h) for c in range(r, h)]
        return rows + squares

    def __repr__(self) -> str:
        return f"NTupleNetwork(size={self.size}, tuples={len(self.tuples)}, weights={self.n_weights})"

    # ------------------------------------------------------------------------------------------------ weights
    def weights_changed(self) -> None:
        """Tell the network that self.weights was written (the pure-Python statement re-reads it)."""
        self._host = None

    def host_weights(self) -> np.ndarray:
        if self._host is None:
            self._host = self.weights.cpu().numpy().copy()
        return self._host

    def fill_hash(self, seed: int) -> "NTupleNetwork":
        """Set every weight from hash_weights(table, index, seed) (its docstring states the formula): the same
        weights wherever they are rebuilt, without storing them."""
        w = np.concatenate([hash_weights(t, 16 ** len(c), seed) for t, c in enumerate(self.tuples)])
        self.weights.copy_(torch.from_numpy(w))
        self.weights_changed()
        return self

    def state_dict(self) -> dict:
        """Plain numpy arrays: size, tuples ([B, 6], padded with -1) and the weights."""
        tup = np.full((len(self.tuples), L.NTUPLE_MAX_CELLS), -1, dtype=np.int64)
        for i, t in enumerate(self.tuples):
            tup[i, :len(t)] = t
        return {"size": np.int64(self.size), "tuples": tup, "weights": self.weights.cpu().numpy().copy()}

    def load_state_dict(self, st) -> None:
        tup = [tuple(int(c) for c in row if c >= 0) for row in np.asarray(st["tuples"])]
        if int(st["size"]) != self.size or tup != self.tuples:
            raise ValueError("the state is of a network with another size or other tuples")
        w = np.asarray(st["weights"])
        if w.dtype != np.int32 or w.shape != (self.n_weights,):
            raise ValueError(f"weights must be {self.n_weights} int32 values")
        self.weights.copy_(torch.from_numpy(np.ascontiguousarray(w)))
        self.weights_changed()

    # ------------------------------------------------------------------------------------------------ device
    def _descriptor(self, depth: int = 0) -> L.NTuple:
        if not self.weights.is_contiguous() or self.weights.dtype != torch.int32 or \
                self.weights.numel() != self.n_weights:
            raise ValueError("weights must stay a contiguous int32 tensor of n_weights entries")
        return L.NTuple(depth, len(self.features), self._feat, self.weights.data_ptr(), self.n_weights)

    def _flat_boards(self, boards: torch.Tensor):
        """(boards as [m] bitboards or [W, m] planes on the device, the shape of the batch, the size argument or ())."""
        if not isinstance(boards, torch.Tensor) or boards.dtype != torch.int64:
            raise ValueError("boards must be an int64 tensor")
        if self.size != 4:
            W = (self.size * self.size + 15) // 16
            if boards.dim() < 1 or boards.shape[0] != W:
                raise ValueError(f"boards of size {self.size} are [{W}, ...] planes (got shape {tuple(boards.shape)})")
            return boards.to(self.device).reshape(W, -1).contiguous(), tuple(boards.shape[1:]), (self.size,)
        return boards.to(self.device).reshape(-1).contiguous(), tuple(boards.shape), ()

    @torch.no_grad()
    def values(self, boards: torch.Tensor) -> torch.Tensor:
        """V of every board (g2048_ntuple_values / g2048_sized_ntuple_values): boards int64, [...] bitboards at size 4
        or [W, ...] planes otherwise; returns int64 [...]."""
        flat, shape, head = self._flat_boards(boards)
        L.ensure_device(self.device)
        m = flat.shape[-1]
        out = torch.empty(m, dtype=torch.int64, device=self.device)
        d = self._descriptor()
        fn = L.lib().g2048_sized_ntuple_values if head else L.lib().g2048_ntuple_values
        L.check(fn(*head, ctypes.byref(d), L.ptr(flat), m, L.ptr(out), L.stream_handle(self.device)))
        return out.view(shape)

    # ------------------------------------------------------------------------------------------------ the statement
    def value(self, exponents) -> int:
        """V of one board of size * size exponents, row-major, in plain Python."""
        w = self.host_weights()
        return sum(int(w[off + sum(int(exponents[c]) << (4 * j) for j, c in enumerate(cells))])
                   for _, off, cells in self.features)


class NTuplePolicy:
    """The player of an NTupleNetwork: greedy on Q_0 (depth 0) or on Q_1, which averages over the tile that spawns next
    (depth 1); the module docstring states both.  It never looks at the action mask (it plays with use_action_mask on
    or off), never chooses an invalid action and never draws from the policy stream.

    Accepted as ``action_gen`` by rollout_batch, evaluate_batch, run_episode and the runner's evaluation_loop, which play
    it on the device (g2048_ntuple_rollout / g2048_ntuple_eval); the weights are read at each call, so training the
    network changes the player.  Also callable with the reference's signature ``(state, action_mask) -> int`` (state:
    the board's tile values), so an instance serves as the ``action_gen`` of the reference itself."""

    def __init__(self, network: NTupleNetwork, depth: int = 0):
        if not isinstance(network, NTupleNetwork):
            raise TypeError(f"network must be an NTupleNetwork (got {type(network).__name__})")
        try:
            if isinstance(depth, bool):
                raise TypeError
            depth = operator.index(depth)
        except TypeError:
            raise ValueError(f"depth must be an integer in 0..{L.NTUPLE_MAX_DEPTH}, got {depth!r}") from None
        if not 0 <= depth <= L.NTUPLE_MAX_DEPTH:
            raise ValueError(f"depth must be an integer in 0..{L.NTUPLE_MAX_DEPTH}, got {depth!r}")
        self.network, self.depth = network, depth

    def __repr__(self) -> str:
        return f"NTuplePolicy({self.network!r}, depth={self.depth})"

    def _ntuple(self) -> L.NTuple:
        return self.network._descriptor(self.depth)

    def _q0(self, b) -> list:
        n, out = self.network.size, []
        for a in range(4):
            m, g = move_score(b, n, a)
            out.append(INVALID_Q if m == b else (g << FRAC_BITS) + self.network.value(m))
        return out

    def _q1(self, b) -> list:
        n, out = self.network.size, []
        for a in range(4):
            m, g = move_score(b, n, a)
            if m == b:
                out.append(INVALID_Q)
                continue
            empty = [c for c in range(n * n) if m[c] == 0]
            total = 0
            for c in empty:
                for e, weight in ((1, 9), (2, 1)):
                    q = [v for v in self._q0(m[:c] + (e,) + m[c + 1:]) if v != INVALID_Q]
                    total += weight * (max(q) if q else 0)
            out.append((g << FRAC_BITS) + total // (10 * len(empty)))
        return out

    def q_values(self, exponents) -> list:
        """[Q_depth(b, a) for a in 0..3], INVALID_Q = -2^63 for an invalid action; exponents: size * size cells."""
        b = tuple(int(e) for e in exponents)
        if len(b) != self.network.size ** 2:
            raise ValueError(f"a board of this network has {self.network.size ** 2} cells (got {len(b)})")
        return self._q1(b) if self.depth else self._q0(b)

    def choose(self, exponents) -> int:
        """The choice on a board of exponents (0 when no action is valid)."""
        q = self.q_values(exponents)
        return max(range(4), key=lambda a: (q[a], -a)) if max(q) != INVALID_Q else 0

    def __call__(self, state, action_mask=None) -> int:
        return self.choose([int(v).bit_length() - 1 if v else 0 for row in state for v in row])
