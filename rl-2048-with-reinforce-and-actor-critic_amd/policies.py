"""Scripted players for ReinforceAgent.rollout_batch / evaluate_batch / run_episode (their ``action_gen`` argument): the
reference's baseline generators (tools/simple_action_gen.py) as objects the device kernels of
include/g2048_scripted.h can play whole episodes for.  No device work happens here."""
from __future__ import annotations

import ctypes
import operator

from . import _lib as L


class PriorityPolicy:
    """The first action of ``order`` (a permutation of (0, 1, 2, 3): 0 up, 1 right, 2 down, 3 left) that the board's
    action mask allows.  PriorityPolicy(PriorityPolicy.URDL) is the reference's action_gen_1 and
    PriorityPolicy(PriorityPolicy.URLD) its action_gen_2.  select_action takes a valid candidate as it is
    (src/reinforce_agent.py:153-176): the policy stream is never drawn from and the net does not influence the episode.

    Callable with the reference's signature ``(state, action_mask) -> int``, so an instance also serves as the
    ``action_gen`` of the host path and of the reference itself."""

    URDL = (0, 1, 2, 3)
    URLD = (0, 1, 3, 2)

    def __init__(self, order):
        try:
            entries = tuple(operator.index(a) for a in order)   # integers only: 1.0 or "1" is no action
        except TypeError:
            raise ValueError(f"order must be a permutation of (0, 1, 2, 3), got {order!r}") from None
        if sorted(entries) != [0, 1, 2, 3]:
            raise ValueError(f"order must be a permutation of (0, 1, 2, 3), got {order!r}")
        self.order = entries

    def __call__(self, state, action_mask) -> int:
        for a in self.order:
            if action_mask[a]:
                return a
        return self.order[0]

    def __repr__(self) -> str:
        return f"PriorityPolicy({self.order!r})"

    def _script(self) -> L.Script:
        return L.Script(L.SCRIPT_PRIORITY, (ctypes.c_uint8 * 4)(*self.order))


class UniformPolicy:
    """The random-valid baseline on the episode's policy stream: select_action for a net whose logits are all equal.
    p[a] = fp32(1) / fp32(k) on the k actions the mask allows (all four when the env has no action mask), 0 elsewhere;
    one Generator.random() draw per step, also when k = 1; the action is Generator.choice(4, p=p).  Not a callable: it
    needs the policy stream, which the reference's action_gen signature does not carry."""

    def __repr__(self) -> str:
        return "UniformPolicy()"

    def _script(self) -> L.Script:
        return L.Script(L.SCRIPT_UNIFORM, (ctypes.c_uint8 * 4)(0, 1, 2, 3))


def _slide(line):
    """One line moved towards its first cell (exponents, 0 = empty): (new line, sum of the merged exponents)."""
    tiles = [e for e in line if e]
    out, gain, i = [], 0, 0
    while i < len(tiles):
        if i + 1 < len(tiles) and tiles[i] == tiles[i + 1]:
            out.append(tiles[i] + 1)
            gain += tiles[i] + 1
            i += 2
        else:
            out.append(tiles[i])
            i += 1
    return out + [0] * (len(line) - len(out)), gain


def _move(b, n, a):
    """move(b, a) without the spawn on a row-major tuple of n x n exponents: (new board, gain)."""
    nb, gain = list(b), 0
    for k in range(n):
        idx = [k * n + j for j in range(n)] if a in (1, 3) else [j * n + k for j in range(n)]
        if a in (1, 2):
            idx.reverse()
        new, g = _slide([b[i] for i in idx])
        gain += g
        for i, v in zip(idx, new):
            nb[i] = v
    return tuple(nb), gain


class ExpectimaxPolicy:
    """A lookahead player: for each move, slide, score the afterstate, and average over the tile that spawns next.
    All integers, so this class, the host build of csrc/g2048_search_core.h and the device kernels of
    include/g2048_search.h agree bit for bit; this class is the readable statement of the player.

    On a board b of n x n exponents (0 = empty), with move(b, a) the env's slide / merge without the spawn and an
    action valid iff it changes the board:

      gain(b, a) = sum of log2(v) over the tiles v created by merges in move(b, a)
      H(b)       = w_empty #empty(b) + w_smooth sum over adjacent cell pairs of (15 - |e_i - e_j|)
                   + w_corner sum_{r,c} e[r][c] ((n-1-r) + (n-1-c))
      C_0(m)     = H(m)
      C_d(m)     = (sum over empty cells c of m of 9 V_{d-1}(m + a 2 at c) + V_{d-1}(m + a 4 at c)) // (10 #empty(m))
      Q_d(b, a)  = w_merge gain(b, a) + C_d(move(b, a))      for valid a
      V_d(b)     = max over valid a of Q_d(b, a), 0 when no action is valid

    The choice is the valid action with the largest Q_depth(b, a), the lowest index among equals.  depth in {0, 1, 2},
    weights integers in 0..4096; the defaults are untuned.  It never looks at the action mask (it plays with
    use_action_mask on or off), never chooses an invalid action and never draws from the policy stream.

    Callable with the reference's signature ``(state, action_mask) -> int`` (state: the board's tile values, as
    Game2048Env.state), so an instance also serves as the ``action_gen`` of the host path and of the reference itself
    -- at seconds per episode; rollout_batch / evaluate_batch / run_episode play it on the device."""

    def __init__(self, depth=1, w_merge=4, w_empty=16, w_smooth=1, w_corner=2):
        def integer(name, v, hi):
            try:
                if isinstance(v, bool):
                    raise TypeError
                v = operator.index(v)           # integers only: 1.0 or "1" is no depth
            except TypeError:
                raise ValueError(f"{name} must be an integer in 0..{hi}, got {v!r}") from None
            if not 0 <= v <= hi:
                raise ValueError(f"{name} must be an integer in 0..{hi}, got {v!r}")
            return v

        self.depth = integer("depth", depth, L.SEARCH_MAX_DEPTH)
        self.w_merge = integer("w_merge", w_merge, L.SEARCH_MAX_WEIGHT)
        self.w_empty = integer("w_empty", w_empty, L.SEARCH_MAX_WEIGHT)
        self.w_smooth = integer("w_smooth", w_smooth, L.SEARCH_MAX_WEIGHT)
        self.w_corner = integer("w_corner", w_corner, L.SEARCH_MAX_WEIGHT)

    def __repr__(self) -> str:
        return (f"ExpectimaxPolicy(depth={self.depth}, w_merge={self.w_merge}, w_empty={self.w_empty}, "
                f"w_smooth={self.w_smooth}, w_corner={self.w_corner})")

    def _search(self) -> L.Search:
        return L.Search(self.depth, self.w_merge, self.w_empty, self.w_smooth, self.w_corner)

    # ------------------------------------------------------------------ the player, on a tuple of n * n exponents
    def heuristic(self, b, n) -> int:
        smooth = corner = 0
        for r in range(n):
            for c in range(n):
                e = b[r * n + c]
                if c + 1 < n:
                    smooth += 15 - abs(e - b[r * n + c + 1])
                if r + 1 < n:
                    smooth += 15 - abs(e - b[(r + 1) * n + c])
                corner += e * ((n - 1 - r) + (n - 1 - c))
        return self.w_empty * sum(1 for e in b if e == 0) + self.w_smooth * smooth + self.w_corner * corner

    def _chance(self, m, n, d) -> int:
        if d == 0:
            return self.heuristic(m, n)
        empty = [c for c in range(n * n) if m[c] == 0]
        total = 0
        for c in empty:
            for e, weight in ((1, 9), (2, 1)):
                total += weight * max([q for q in self._q(m[:c] + (e,) + m[c + 1:], n, d - 1) if q >= 0], default=0)
        return total // (10 * len(empty))

    def _q(self, b, n, d) -> list:
        out = []
        for a in range(4):
            m, gain = _move(b, n, a)
            out.append(-1 if m == b else self.w_merge * gain + self._chance(m, n, d))
        return out

    def q_values(self, exponents) -> list:
        """[Q_depth(b, a) for a in 0..3], -1 for an invalid action; exponents: n * n cells, row-major."""
        b = tuple(int(e) for e in exponents)
        n = int(round(len(b) ** 0.5))
        if n * n != len(b) or not 2 <= n <= 8:
            raise ValueError(f"a board is n x n cells, 2 <= n <= 8 (got {len(b)} cells)")
        return self._q(b, n, self.depth)

    def choose(self, exponents) -> int:
        """The choice on a board of exponents (0 when no action is valid)."""
        q = self.q_values(exponents)
        return max(range(4), key=lambda a: (q[a], -a)) if max(q) >= 0 else 0

    def __call__(self, state, action_mask=None) -> int:
        return self.choose([int(v).bit_length() - 1 if v else 0 for row in state for v in row])
