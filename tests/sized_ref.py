"""A plain NumPy restatement of the reference game and env (Game2048 + Game2048Env) for any board size 2..8, and the
late-game board families the sized tests share.

It is written from the reference's behaviour (src/game2048.py, src/env.py) and shares no code with
csrc/g2048_sized_core.h: the board is an int64 array of tile values, a move is np.rot90 + a Python row slide that
collects the merged values in order, a spawn draws from a real np.random.Generator(np.random.PCG64(seed))
(integers(len(empties)) over np.argwhere order, then random() < 0.9), and the reward is the fp64 operation order
of src/env.py:197-261.  tests/test_sized_ref_cpu.py pins it to the real reference bit for bit on
tests/golden/sized.npz and tests/golden/sized_late.npz; the GPU tests (tests/test_gpu_sized_late.py) then use it on
states no fixture holds.

saturate=True models the one documented deviation of the kernels: the nibble board holds 2^15
where a 2^15 + 2^15 merge made 65536; the merged list, score, reward and max_tile_seen still carry the true 65536.
Done, mask, obs and the empty count are then those of the saturated board.
"""
from __future__ import annotations

import numpy as np

ENV_DEFAULTS = dict(obs_mode="raw", obs_log2_scale=1.0, reward_mode="sum", base_reward_scale=1.0,
                    empty_tile_reward=0.0, merge_reward=0.0, bonus_mode="off", bonus_scale=1.0, step_reward=0.0,
                    endgame_penalty=0.0, use_action_mask=True, invalid_action_penalty=-1.0, max_steps=1024)

# the two configs of the bulk differential: the log2 reward with every bonus term, and raw obs without action mask
# with max_steps None
BULK_CFGS = {
    "log2_all": dict(obs_mode="log2", obs_log2_scale=0.1, reward_mode="log2", base_reward_scale=0.1,
                     empty_tile_reward=0.05, merge_reward=0.3, bonus_mode="log2", bonus_scale=0.7, step_reward=-0.01,
                     endgame_penalty=-10.0, max_steps=150),
    "raw_nomask": dict(obs_mode="raw", use_action_mask=False, reward_mode="sum", empty_tile_reward=0.1,
                       max_steps=None),
}
BULK_LANES, BULK_STEPS = 1031, 6
PHILOX_TWO = 3865470566          # a Philox spawn is a 2 iff y < 0.9 * 2**32


# ------------------------------------------------------------------------------------------------ value <-> exponent
def values(e) -> np.ndarray:
    e = np.asarray(e, dtype=np.int64)
    return np.where(e > 0, np.int64(1) << e, 0).astype(np.int64)


def exponents(v) -> np.ndarray:
    """Tile values (0 or powers of two up to 65536) -> uint8 exponents, same shape."""
    v = np.asarray(v, dtype=np.int64)
    e = np.zeros(v.shape, dtype=np.uint8)
    for k in range(1, 17):
        e[v == (1 << k)] = k
    assert np.array_equal(values(e), v), "not a board of powers of two"
    return e


def words(n: int) -> int:
    return (n * n + 15) // 16


def pack_planes(e: np.ndarray, n: int) -> np.ndarray:
    """uint8 exponents [m, N*N] -> int64 planes [W, m] (cell k: nibble k & 15 of word k >> 4)."""
    e = np.asarray(e, dtype=np.uint64).reshape(-1, n * n)
    out = np.zeros((words(n), e.shape[0]), dtype=np.uint64)
    for k in range(n * n):
        out[k >> 4] |= e[:, k] << np.uint64(4 * (k & 15))
    return out.view(np.int64)


def unpack_planes(p: np.ndarray, n: int) -> np.ndarray:
    """int64 planes [W, ...] -> uint8 exponents [..., N*N]."""
    p = np.asarray(p).view(np.uint64)
    return np.stack([(p[k >> 4] >> np.uint64(4 * (k & 15))) & np.uint64(15) for k in range(n * n)],
                    axis=-1).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------ game
def slide_row(row: list[int]) -> tuple[list[int], list[int]]:
    """One row towards index 0: tiles close up, an equal pair becomes one tile of twice the value (each tile merges
    once, leftmost pair first).  Returns the new row and the merged values in order."""
    tiles = [v for v in row if v]
    out, merged, i = [], [], 0
    while i < len(tiles):
        if i + 1 < len(tiles) and tiles[i] == tiles[i + 1]:
            out.append(2 * tiles[i])
            merged.append(2 * tiles[i])
            i += 2
        else:
            out.append(tiles[i])
            i += 1
    return out + [0] * (len(row) - len(out)), merged


def move(board: np.ndarray, action: int) -> tuple[np.ndarray, list[int], bool]:
    """Action 0 up, 1 right, 2 down, 3 left.  The board is turned clockwise 3 - action times, every row slid left top
    to bottom (which fixes the order of the merged list), and turned back.  Returns (board, merged, changed)."""
    turned = np.rot90(board, k=action - 3)
    rows, merged = [], []
    for r in turned.tolist():
        nr, m = slide_row(r)
        rows.append(nr)
        merged += m
    out = np.rot90(np.array(rows, dtype=np.int64), k=3 - action)
    return np.ascontiguousarray(out), merged, not np.array_equal(out, board)


def is_done(board: np.ndarray) -> bool:
    if (board == 0).any():
        return False
    return not ((board[:, :-1] == board[:, 1:]).any() or (board[:-1] == board[1:]).any())


def action_mask(board: np.ndarray) -> list[int]:
    return [int(move(board, a)[2]) for a in range(4)]


def mask_bits(m) -> int:
    return int(sum(int(b) << i for i, b in enumerate(m)))


def obs_of(board: np.ndarray, mode: str, scale: float = 1.0) -> np.ndarray:
    """The env's board observation, flattened: float32 [N*N] (raw / log2) or [N*N*17] (onehot).  board: tile values
    [..., N, N]; leading axes are kept."""
    b = np.asarray(board, dtype=np.int64)
    lead = b.shape[:-2]
    if mode == "raw":
        return b.astype(np.float32).reshape(*lead, -1)
    e = exponents(b)
    if mode == "log2":
        x = e.astype(np.float32)
        x *= scale
        return x.reshape(*lead, -1)
    if mode == "onehot":
        return np.eye(17, dtype=np.float32)[e.astype(np.int64)].reshape(*lead, -1)
    raise ValueError(mode)


def symmetries(board: np.ndarray, action: int, mask=None) -> list[tuple]:
    """The 8 dihedral images in get_symmetries order: the board turned counter-clockwise 0..3 times, then its
    left-right mirror turned 0..3 times; each with the action (and the action mask, if given) that means the same
    move on the image.  board: [N, N] or [N, N, C] (the first two axes turn)."""
    out = []
    for flip in (False, True):
        b = np.fliplr(board) if flip else board
        a = {1: 3, 3: 1}.get(action, action) if flip else action
        m = None if mask is None else (np.asarray(mask)[[0, 3, 2, 1]] if flip else np.asarray(mask))
        for k in range(4):
            out.append((np.rot90(b, k=k, axes=(0, 1)).copy(), (a - k) % 4, None if m is None else np.roll(m, -k)))
    return out


def philox_spawn(board: np.ndarray, seed: int, key: int, counter: int, tag: int, second: bool = False) -> None:
    """The Philox spawn rule (tests/test_sized_host.py::test_philox_draw_and_spawn_rule): Philox4x32-10 on counter
    (seed lo, seed hi, counter, tag) keyed by the key halves; cell (x * n_empty) >> 32 in row-major order of the
    empties gets a 2 iff y < 3865470566, else a 4.  second: use (z, w) in place of (x, y)."""
    from oracle import oracle as O

    empt = np.argwhere(board == 0)
    if len(empt) == 0:
        return
    d = [int(v) for v in O.philox4x32_10((seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, counter, tag),
                                         (key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF))]
    x, y = (d[2], d[3]) if second else (d[0], d[1])
    r, c = empt[(x * len(empt)) >> 32]
    board[r, c] = 2 if y < PHILOX_TWO else 4


class SizedRef:
    """One Game2048Env of size n (cfg: the env config's fields as a dict) with every piece of state open to the
    test: board (tile values), steps, max_tile_seen, score, and the bit generator's state."""

    def __init__(self, n: int, cfg: dict | None = None, saturate: bool = False, rng: str = "pcg64",
                 philox_key: int = 0x2048):
        self.n = n
        self.cfg = dict(ENV_DEFAULTS)
        self.cfg.update(cfg or {})
        self.saturate = saturate
        self.rng = rng
        self.key = philox_key
        self.board = np.zeros((n, n), dtype=np.int64)
        self.steps, self.score, self.max_tile_seen, self.seed = 0, 0, 4, 0
        self.gen = None

    # ---- state
    def reset(self, seed: int) -> None:
        self.seed = int(seed)
        self.board = np.zeros((self.n, self.n), dtype=np.int64)
        self.steps, self.score, self.max_tile_seen = 0, 0, 4
        if self.rng == "pcg64":
            self.gen = np.random.Generator(np.random.PCG64(self.seed))
            self._spawn()
            self._spawn()
        else:
            philox_spawn(self.board, self.seed, self.key, 0, 1)
            philox_spawn(self.board, self.seed, self.key, 0, 1, second=True)

    def inject(self, board=None, steps=None, max_tile_seen=None) -> None:
        """Overwrite the board (tile values [N, N]), the env's step count and / or max_tile_seen."""
        if board is not None:
            self.board = np.array(board, dtype=np.int64).reshape(self.n, self.n)
        if steps is not None:
            self.steps = int(steps)
        if max_tile_seen is not None:
            self.max_tile_seen = int(max_tile_seen)

    @property
    def rng_state(self) -> dict:
        """The PCG64 state as the lane buffers hold it: 128-bit state and inc, the buffered-uint32 flag and value."""
        s = self.gen.bit_generator.state
        return dict(state=int(s["state"]["state"]), inc=int(s["state"]["inc"]), has_uint32=int(s["has_uint32"]),
                    uinteger=int(s["uinteger"]))

    @rng_state.setter
    def rng_state(self, d: dict) -> None:
        s = self.gen.bit_generator.state
        s["state"] = dict(state=int(d["state"]), inc=int(d["inc"]))
        s["has_uint32"], s["uinteger"] = int(d["has_uint32"]), int(d["uinteger"])
        self.gen.bit_generator.state = s

    # ---- game
    def _spawn(self) -> None:
        empt = np.argwhere(self.board == 0)
        if len(empt) == 0:
            return
        r, c = empt[self.gen.integers(len(empt))]
        self.board[r, c] = 2 if self.gen.random() < 0.9 else 4

    def mask(self) -> list[int]:
        return action_mask(self.board)

    def obs(self) -> np.ndarray:
        return obs_of(self.board, self.cfg["obs_mode"], self.cfg["obs_log2_scale"])

    def _reward(self, merged: list[int], done: bool, invalid: bool) -> float:
        c = self.cfg
        if not c["use_action_mask"] and invalid:
            return c["invalid_action_penalty"]
        if c["reward_mode"] == "sum":
            reward = float(sum(merged))
        elif c["reward_mode"] == "log2":
            reward = 0.0
            for v in merged:
                reward += float(np.log2(v))
        else:
            raise ValueError(c["reward_mode"])
        reward *= c["base_reward_scale"]
        if c["empty_tile_reward"] != 0.0:
            reward += c["empty_tile_reward"] * float(np.sum(self.board == 0))
        if c["merge_reward"] != 0.0:
            reward += c["merge_reward"] * float(len(merged))
        top = max(merged, default=0)
        if top >= 8 and top > self.max_tile_seen:
            bonus = {"off": 0.0, "raw": float(top), "log2": float(np.log2(top))}[c["bonus_mode"]]
            self.max_tile_seen = top
            bonus *= c["bonus_scale"]
            reward += bonus
        reward += c["step_reward"]
        if done and c["endgame_penalty"] != 0.0:
            reward += c["endgame_penalty"]
        return reward

    def step(self, action: int) -> dict:
        self.steps += 1
        new, merged, changed = move(self.board, action)
        sat = 65536 in merged
        if self.saturate:
            new = np.minimum(new, 32768)
        self.board = new
        done = is_done(new)
        self.score += sum(merged)
        if changed:
            if self.rng == "pcg64":
                self._spawn()
            else:
                philox_spawn(self.board, self.seed, self.key, self.steps, 0)
            done = is_done(self.board)
        invalid = (not changed) and (not done)
        reward = self._reward(merged, done, invalid)
        ms = self.cfg["max_steps"]
        truncated = ms is not None and self.steps >= ms and not done
        return dict(changed=changed, terminated=bool(done), truncated=bool(truncated), invalid=bool(invalid),
                    reward=reward, merged=merged, score=self.score, step_index=self.steps,
                    max_tile_seen=self.max_tile_seen, saturated=sat)


def pad_merged(merged: list[int], n: int) -> np.ndarray:
    """The merged values as the kernels' list: exponents in order, zero-padded to N * (N // 2)."""
    out = np.zeros(n * (n // 2), dtype=np.uint8)
    out[:len(merged)] = [int(v).bit_length() - 1 for v in merged]
    return out


# ------------------------------------------------------------------------------------------------- board families
LINES = ([14, 14], [15, 15], [15] * 8, [14, 14, 15, 15], [15, 0, 15], [13, 13, 14, 14])


def straddle_rows(n: int) -> list[int]:
    """Rows whose cells lie in two 64-bit words (cell k is in word k >> 4)."""
    return [r for r in range(n) if (r * n) >> 4 != (r * n + n - 1) >> 4]


def _line(k: int, n: int) -> np.ndarray:
    ln = list(LINES[k])
    if k in (3, 4, 5):                       # the open-ended lines go on with their own pattern
        ln = (ln * 4)[:n]
    ln = (ln + [0] * n)[:n]
    return np.array(ln, dtype=np.int64)


def _no_merge(n: int) -> np.ndarray:
    """A full board without equal neighbours, mixing low and high exponents: neighbours differ in (r + c) parity,
    one parity holds 1..3 and the other 9..13."""
    r, c = np.indices((n, n))
    return np.where((r + c) % 2 == 0, 1 + (3 * r + c) % 3, 9 + (r + 2 * c) % 5).astype(np.int64)


DENSE_P = np.array([0.0] + [0.2 / 7] * 7 + [0.68 / 6] * 6 + [0.08, 0.04])   # exponents 1..15, weight on 8..15


def _dense(rng, n: int, n_empty: int, loose: bool) -> np.ndarray:
    """Exponents weighted towards 8..15 with n_empty empty cells.  loose: equal neighbours are left as drawn; else
    every cell is redrawn until it differs from its left and upper neighbours (a board about to end)."""
    e = rng.choice(16, size=(n, n), p=DENSE_P).astype(np.int64)
    if not loose:
        for r in range(n):
            for c in range(n):
                while (c and e[r, c] == e[r, c - 1]) or (r and e[r, c] == e[r - 1, c]):
                    e[r, c] = rng.choice(16, p=DENSE_P)
    cells = rng.permutation(n * n)[:n_empty]
    e.reshape(-1)[cells] = 0
    return e


def family_boards(n: int, seed: int, dense: int = 8) -> list[tuple[str, np.ndarray]]:
    """The late-game board families at size n as (name, uint8 exponents [N*N]), in a fixed order.  ``dense`` random
    boards follow the crafted ones (the fixture generator uses 8; the bulk differential fills its lanes with them)."""
    rng = np.random.default_rng([seed, n])
    out: list[tuple[str, np.ndarray]] = []
    # explicit lines: every line in every word-straddling row (rows 0 and N-1 where one word holds the board or no
    # row straddles) and one column, forwards and reversed in turn, over a sparse low background
    rows = straddle_rows(n) or [0, n - 1]
    for where in [("r", r) for r in rows] + [("c", n // 2)]:
        for k in range(len(LINES)):
            b = rng.integers(1, 8, size=(n, n))
            b[rng.random((n, n)) < 0.3] = 0
            ln = _line(k, n)
            ln = ln[::-1] if (k + where[1]) % 2 else ln
            if where[0] == "r":
                b[where[1], :] = ln
            else:
                b[:, where[1]] = ln
            out.append((f"line{k}_{where[0]}{where[1]}", b))
    # one empty cell: the first and last nibble of every word, in a no-merge pattern
    for cell in sorted({0, n * n - 1} | {k for k in (15, 16, 31, 32, 47, 48) if k < n * n}):
        b = _no_merge(n)
        b.reshape(-1)[cell] = 0
        out.append((f"hole{cell}", b))
    # terminal and near-terminal: checkerboards of two high exponents, then one equal pair in the last row / column
    r, c = np.indices((n, n))
    for lo, hi in ((12, 13), (14, 15)):
        out.append((f"checker{lo}", np.where((r + c) % 2 == 0, lo, hi)))
    ck = np.where((r + c) % 2 == 0, 12, 13)    # the pair merges to 14 or less: the episode goes on to its end
    b = ck.copy()
    b[n - 1, n - 1] = b[n - 1, n - 2]
    b[n - 2, n - 1] = 10                       # it was equal to the new corner; 10 differs from all its neighbours
    out.append(("pair_row", b))
    b = ck.copy()
    b[n - 1, n - 1] = b[n - 2, n - 1]
    b[n - 1, n - 2] = 10
    out.append(("pair_col", b))
    # full merged list: every cell equal; rows (columns) of equal tiles with distinct rows (columns)
    for e in (1, 14, 15):
        out.append((f"all{e}", np.full((n, n), e)))
    out.append(("eq_rows", np.tile(8 + np.arange(n)[:, None], (1, n))))
    out.append(("eq_cols", np.tile(8 + np.arange(n)[None, :], (n, 1))))
    # dense high tiles with 0..3 empty cells, loose and tight in turn
    for i in range(dense):
        out.append((f"dense{i % 4}{'t' if (i // 4) % 2 else 'l'}", _dense(rng, n, i % 4, (i // 4) % 2 == 0)))
    return [(name, np.asarray(b, dtype=np.uint8).reshape(-1)) for name, b in out]


def late_coverage(data, n: int) -> dict:
    """What the late-game fixture (the arrays of sized_late.npz) holds at size n, summed over its configs: steps that
    terminate, spawns into a single empty cell, 14+14 merges, saturated merges, moves that fill the merged list,
    steps with max_tile_seen >= 2^15, and the episodes per word-straddling row."""
    cov = dict(terminated=0, single_empty_spawn=0, merge_14_14=0, saturated=0, full_list=0, max_tile_2p15=0)
    rows = {r: 0 for r in straddle_rows(n)}
    fam = [str(s) for s in data[f"n{n}_fam"]]
    for c in (int(x) for x in data["env_sel"]):
        p = f"n{n}_c{c}_"
        mer = data[p + "merged"]
        cov["terminated"] += int(data[p + "terminated"].sum())
        cov["merge_14_14"] += int((mer == 15).any(axis=1).sum())
        cov["saturated"] += int((mer == 16).any(axis=1).sum())
        cov["full_list"] += int((mer[:, -1] != 0).sum())
        cov["max_tile_2p15"] += int((data[p + "max_tile_seen"] >= 1 << 15).sum())
        for e, (start, ln) in enumerate(zip(data[p + "ep_start"], data[p + "ep_len"])):
            for r in rows:
                rows[r] += fam[e].startswith("line") and fam[e].endswith(f"_r{r}")
            prev = data[p + "ep_board"][e]
            for j in range(int(start), int(start + ln)):
                moved, _, changed = move(values(prev).reshape(n, n), int(data[p + "action"][j]))
                cov["single_empty_spawn"] += bool(changed and (moved == 0).sum() == 1)
                prev = data[p + "board"][j]
    cov["straddle_rows"] = rows
    return cov


def late_coverage_ok(cov: dict, n: int) -> bool:
    """The coverage every size must have.  N = 2 (one word, a 2-slot list) has no straddling row; everything else
    -- termination, the one-empty-cell spawn, 14+14, a saturated merge, a full (2-slot) list, max_tile_seen >= 2^15
    -- is required of it as of every other size."""
    need = ("terminated", "single_empty_spawn", "merge_14_14", "saturated", "full_list", "max_tile_2p15")
    return all(cov[k] >= 1 for k in need) and all(v >= 1 for v in cov["straddle_rows"].values())


def bulk_setup(n: int, cfg_name: str):
    """The bulk differential's inputs at size n: boards [lanes, N*N], seeds, actions [steps, lanes], the
    max_tile exponent (0 = leave) and step count (-1 = leave) planted per lane.  One definition for the GPU test and
    the CPU cap check."""
    cfg = BULK_CFGS[cfg_name]
    fam = family_boards(n, 7000 + n, dense=BULK_LANES)
    boards = np.stack([b for _, b in fam])[:BULK_LANES]           # every crafted family, then dense boards
    assert boards.shape == (BULK_LANES, n * n)
    rng = np.random.default_rng([n, len(cfg_name)])
    seeds = [int(s) for s in rng.integers(0, 2**63, size=BULK_LANES)]
    actions = rng.integers(0, 4, size=(BULK_STEPS, BULK_LANES)).astype(np.uint8)
    lane = np.arange(BULK_LANES)
    maxt = np.where(lane % 3 == 0, rng.integers(8, 16, size=BULK_LANES), 0)
    ms = cfg["max_steps"]
    near = (ms - 1) if ms is not None else 500000                 # max_steps None: a large count that never truncates
    stepc = np.where(lane % 3 == 1, near - rng.integers(0, 3, size=BULK_LANES), -1)
    return boards, seeds, actions, maxt, stepc


def bulk_refs(n: int, cfg_name: str):
    """The reference lanes of bulk_setup, ready to step (saturate=True: the kernels' board contract)."""
    boards, seeds, actions, maxt, stepc = bulk_setup(n, cfg_name)
    refs = []
    for i in range(BULK_LANES):
        r = SizedRef(n, BULK_CFGS[cfg_name], saturate=True)
        r.reset(seeds[i])
        r.inject(values(boards[i]), steps=None if stepc[i] < 0 else int(stepc[i]),
                 max_tile_seen=None if maxt[i] == 0 else 1 << int(maxt[i]))
        refs.append(r)
    return refs, boards, seeds, actions, maxt, stepc


LEMIRE_LANES = 519


def lemire_setup(n: int):
    """Inputs of the Lemire-fallback test at size n: boards with 1 .. N*N - 1 empty cells, seeds, two rounds of
    actions, and per lane the buffered uint32 to plant (-1 = none).  integers(n_empty) takes next_uint32() * n_empty,
    and only if that product's low word is below n_empty does it compute the threshold 2^32 mod n_empty and reject
    (redraw) below it.  A planted 0 has low word 0: rejected unless n_empty is a power of two; a planted
    ceil(2^32 / n_empty) has low word n_empty - 2^32 mod n_empty.  Returns (boards, seeds, actions, plant, stats)."""
    L = LEMIRE_LANES
    rng = np.random.default_rng(31 + n)
    fill = rng.choice([0.05, 0.3, 0.6, 0.9], size=L)
    boards = rng.integers(1, 12, size=(L, n * n)).astype(np.uint8)
    boards[rng.random((L, n * n)) >= fill[:, None]] = 0
    boards[:, 0] = np.maximum(boards[:, 0], 1)
    seeds = [int(s) for s in rng.integers(0, 2**63, size=L)]
    actions = rng.integers(0, 4, size=(2, L)).astype(np.uint8)
    plant = np.full(L, -1, dtype=np.int64)
    stats = dict(accepted=0, rejected=0, sizes=set())
    for i in range(L):
        moved, _, changed = move(values(boards[i]).reshape(n, n), int(actions[0, i]))
        ne = int((moved == 0).sum())
        if not changed or ne < 2 or i % 8 == 7:          # one empty cell draws nothing; some lanes stay plain
            continue
        x = 0 if (ne & (ne - 1) == 0 or rng.integers(2)) else -(-(1 << 32) // ne)
        low = (x * ne) & 0xFFFFFFFF
        assert low < ne                                   # the fallback is entered
        rejected = low < (1 << 32) % ne
        stats["rejected" if rejected else "accepted"] += 1
        stats["sizes"].add(ne)
        plant[i] = x
    return boards, seeds, actions, plant, stats


def as_sized4(env, L=None):
    """Re-point a size-4 VecGame2048Env at the sized entry points (W = 1): same buffers, the sized output struct."""
    import torch

    n = env.n
    env._sized = True
    env.board = env.board.view(1, n)
    env.merged = torch.zeros(n, 8, dtype=torch.uint8, device=env.device)
    env.prev_board = torch.zeros(1, n, dtype=torch.int64, device=env.device)
    env._out = env._sized_out(env.reward, env.flags, env.prev_board, True, env.reward64)
    return env
