"""An independent statement of the n-tuple value network of include/g2048_ntuple.h, for tests/test_ntuple_sizes_cpu.py
and tests/test_gpu_ntuple_sizes.py.  Not a test module.

Written from the header's text alone, on row-major exponent arrays and Python / int64 integers: it includes neither
csrc/g2048_ntuple_core.h (what the kernels AND the host build tests/native/ntuple_host.cpp compile) nor
rl2048_amd.ntuple (the package's Python statement), and the move is its own slide.  A network is a plain list of
features [(offset, cells)] -- the flat list the device reads, symmetry images included or not -- and an int32 weight
array.  The table gathers are vectorised with numpy; the move runs per row (one slide per distinct line is cached).

  values(features, weights, ex)                       V of every board
  q_values(features, weights, size, depth, ex)        (Q_depth [m, 4], choices [m])
  td_update(features, weights, size, ex, actions, flags, lengths, lr_num, lr_shift)
                                                      (weights after, rows, sum |d|, info)

The one thing the header leaves to the env it names ("the env's slide / merge"): a 2^15 + 2^15 merge leaves 2^15 on the
nibble board while its gain is the true 65536.
"""
import functools

import numpy as np

FRAC_BITS = 10
INVALID = -(1 << 63)
STEP_CLAMP = 1 << 30
F_TERMINATED = 0x02


# ------------------------------------------------------------------------------------------------------------ move
@functools.lru_cache(maxsize=1 << 18)
def _slide(line: tuple) -> tuple:
    """One line towards its first cell: (new line, gain).  Tiles close up; the first equal pair from the front merges,
    each tile once."""
    tiles = [e for e in line if e]
    out, gain, i = [], 0, 0
    while i < len(tiles):
        if i + 1 < len(tiles) and tiles[i] == tiles[i + 1]:
            out.append(min(tiles[i] + 1, 15))
            gain += 2 << tiles[i]
            i += 2
        else:
            out.append(tiles[i])
            i += 1
    return tuple(out) + (0,) * (len(line) - len(out)), gain


@functools.lru_cache(maxsize=None)
def _lines(size: int, a: int) -> tuple:
    """The cell indices of every line of action a (0 up, 1 right, 2 down, 3 left), each from the side tiles move to."""
    if a == 0:
        return tuple(tuple(r * size + c for r in range(size)) for c in range(size))
    if a == 2:
        return tuple(tuple(r * size + c for r in reversed(range(size))) for c in range(size))
    if a == 3:
        return tuple(tuple(r * size + c for c in range(size)) for r in range(size))
    return tuple(tuple(r * size + c for c in reversed(range(size))) for r in range(size))


def move(b, size: int, a: int):
    """move(b, a) without the spawn on size * size exponents: (new board as a tuple, gain, changed)."""
    b = tuple(int(e) for e in b)
    nb, gain = list(b), 0
    for idx in _lines(size, a):
        new, g = _slide(tuple(b[i] for i in idx))
        gain += g
        for i, e in zip(idx, new):
            nb[i] = e
    nb = tuple(nb)
    return nb, gain, nb != b


# ---------------------------------------------------------------------------------------------------------- values
def _as_boards(ex) -> np.ndarray:
    ex = np.asarray(ex, dtype=np.int64)
    return ex.reshape(1, -1) if ex.ndim == 1 else ex.reshape(len(ex), -1)


def feature_indices(features, ex) -> np.ndarray:
    """offset_f + index_f(board) for every board and feature: int64 [m, nf]."""
    ex = _as_boards(ex)
    out = np.empty((len(ex), len(features)), dtype=np.int64)
    for f, (off, cells) in enumerate(features):
        idx = np.zeros(len(ex), dtype=np.int64)
        for j, c in enumerate(cells):
            idx += ex[:, c] << (4 * j)
        out[:, f] = off + idx
    return out


def values(features, weights, ex) -> np.ndarray:
    """V of every board of ex [m, N*N] (or one board [N*N]): int64 [m]."""
    w = np.asarray(weights)
    return w[feature_indices(features, ex)].astype(np.int64).sum(axis=1)


def _q0(features, weights, size, ex):
    """Q_0 as Python lists: q [m][4] (INVALID for an invalid action)."""
    ex = _as_boards(ex)
    after, gains, where = [], [], []
    for i, b in enumerate(ex.tolist()):
        for a in range(4):
            m, g, changed = move(b, size, a)
            if changed:
                after.append(m)
                gains.append(g)
                where.append((i, a))
    q = [[INVALID] * 4 for _ in range(len(ex))]
    if after:
        v = values(features, weights, np.array(after, dtype=np.int64)).tolist()
        for (i, a), g, vm in zip(where, gains, v):
            q[i][a] = (g << FRAC_BITS) + vm
    return q


def _best(q4) -> int:
    """V': the largest valid entry, 0 when none is valid."""
    ok = [v for v in q4 if v != INVALID]
    return max(ok) if ok else 0


def q_values(features, weights, size: int, depth: int, ex):
    """(q int64 [m, 4], choices uint8 [m]) at depth 0 or 1 on ex [m, N*N]."""
    ex = _as_boards(ex)
    if depth == 0:
        q = _q0(features, weights, size, ex)
    else:
        assert depth == 1
        q = [[INVALID] * 4 for _ in range(len(ex))]
        succ, plan = [], []                      # every board one spawn after every valid afterstate, in one batch
        for i, b in enumerate(ex.tolist()):
            for a in range(4):
                m, g, changed = move(b, size, a)
                if not changed:
                    continue
                empty = [c for c in range(size * size) if m[c] == 0]
                assert empty                     # a valid move always leaves an empty cell
                plan.append((i, a, g, len(empty), len(succ)))
                for c in empty:
                    for e in (1, 2):
                        succ.append(m[:c] + (e,) + m[c + 1:])
        sq = _q0(features, weights, size, np.array(succ, dtype=np.int64)) if succ else []
        for i, a, g, ne, s in plan:
            total = 0
            for k in range(ne):
                total += 9 * _best(sq[s + 2 * k]) + _best(sq[s + 2 * k + 1])
            q[i][a] = (g << FRAC_BITS) + total // (10 * ne)          # Python's // floors
    acts = np.zeros(len(ex), dtype=np.uint8)
    for i, q4 in enumerate(q):
        best = None
        for a in range(4):
            if q4[a] != INVALID and (best is None or q4[a] > q4[best]):
                best = a                          # strictly larger only: the lowest action wins ties
        acts[i] = 0 if best is None else best
    return np.array(q, dtype=np.int64).reshape(len(ex), 4), acts


# -------------------------------------------------------------------------------------------------------------- TD
def td_update(features, weights, size: int, ex, actions, flags, lengths, lr_num: int, lr_shift: int):
    """One TD(0) update on a time-major batch: ex [T, n, N*N] exponents, actions / flags [T, n], lengths [n] (clamped
    to 0..T).  Returns (weights after as int32 -- `weights` is not written --, rows updated, sum |d|, info); info
    counts what the update met: rows clamped at +2^30 ("clamp_hi") and at -2^30 ("clamp_lo"), rows whose step is 0
    ("zero_steps"), entries whose exact sum left int32 ("wrapped"), the largest number of rows that add to one entry
    ("max_rows_on_entry"), the entries written ("entries") and the row indices t n + i updated ("row_index")."""
    ex = np.asarray(ex, dtype=np.int64)
    T, n = ex.shape[:2]
    actions, flags = np.asarray(actions).reshape(T, n), np.asarray(flags).reshape(T, n)
    lens = [min(max(int(x), 0), T) for x in np.asarray(lengths).tolist()]
    w = np.asarray(weights)
    assert w.dtype == np.int32
    # m_t and g_t of every valid row; an invalid recorded action leaves the board and gains nothing
    rows_ti, after, gains = [], [], []
    for i in range(n):
        for t in range(lens[i]):
            m, g, changed = move(ex[t, i].tolist(), size, int(actions[t, i]) & 3)
            assert changed or g == 0
            rows_ti.append((t, i))
            after.append(m)
            gains.append(g)
    info = dict(clamp_hi=0, clamp_lo=0, zero_steps=0, wrapped=0, max_rows_on_entry=0, entries=0,
                row_index=np.zeros(0, dtype=np.int64))
    new = w.copy()
    if not rows_ti:
        return new, 0, 0, info
    after = np.array(after, dtype=np.int64)
    fidx = feature_indices(features, after)                                   # [R, nf]
    v = w[fidx].astype(np.int64).sum(axis=1).tolist()                         # V(m_t) on the weights before
    q = {ti: (g << FRAC_BITS) + vm for ti, g, vm in zip(rows_ti, gains, v)}
    used, steps = [], []
    rows = abs_delta = 0
    for r, (t, i) in enumerate(rows_ti):
        if t < lens[i] - 1:
            y = q[(t + 1, i)]
        elif int(flags[t, i]) & F_TERMINATED:
            y = 0
        else:
            continue                                                          # a truncated last row
        d = y - v[r]
        rows += 1
        abs_delta += abs(d)
        s = (d * lr_num) >> lr_shift                                          # Python's >> floors
        if s > STEP_CLAMP:
            s = STEP_CLAMP
            info["clamp_hi"] += 1
        elif s < -STEP_CLAMP:
            s = -STEP_CLAMP
            info["clamp_lo"] += 1
        info["zero_steps"] += s == 0
        used.append(r)
        steps.append(s)
    info["row_index"] = np.array([rows_ti[r][0] * n + rows_ti[r][1] for r in used], dtype=np.int64)
    if used:
        hit = fidx[used]                                                      # [U, nf]
        entries, inv = np.unique(hit.reshape(-1), return_inverse=True)
        inv = inv.reshape(-1)
        add = np.zeros(len(entries), dtype=np.int64)                          # |sum| <= 2^30 * U * nf: exact in int64
        np.add.at(add, inv, np.repeat(np.array(steps, dtype=np.int64), hit.shape[1]))
        exact = w[entries].astype(np.int64) + add
        info["wrapped"] = int(((exact < -(1 << 31)) | (exact > (1 << 31) - 1)).sum())
        new[entries] = (((exact + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)).astype(np.int32)
        info["entries"] = int(len(entries))
        # rows (with a non-zero step: a zero step adds nothing) per entry, a row counted once per entry
        live = np.repeat(np.array(steps, dtype=np.int64) != 0, hit.shape[1])
        pair = np.unique(inv[live] * len(used) + np.repeat(np.arange(len(used)), hit.shape[1])[live])
        if len(pair):
            info["max_rows_on_entry"] = int(np.bincount(pair // len(used)).max())
    return new, rows, abs_delta, info
