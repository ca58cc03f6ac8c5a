"""Replay of every episode of a rollout batch in the CPU oracles, shared by tests/test_rollout_replay_cpu.py (which
pins this module: it must pass true batches and fail corrupted ones) and tests/test_gpu_rollout_replay.py (which holds
the persistent rollout kernels to it).

A batch is anything with TrajectoryBatch's fields (boards, actions, rewards, flags, lengths, total_reward, max_tile,
final_boards, probs) as torch tensors or NumPy arrays.  Every valid row (t < lengths[e]) of every episode is compared,
with == only; nothing is sampled and no lane is excluded.

* replay_4x4: teacher-forced through oracle.EnvBatch (one C call per time row; lanes past their end get action 255,
  which the oracle skips).
* replay_sized: the same comparisons per episode in tests/sized_ref.SizedRef.
* check_choices: the recorded action from the recorded probabilities -- a vectorised restatement of numpy's
  Generator.choice(4, p) on the policy stream, or the first argmax of p * mask when greedy.
* check_probs: the recorded probabilities against an fp64 masked softmax of an fp64 forward of the agent's parameters,
  within the forward's fp32 error bound (test_gpu_deep._fwd64_bound) plus 8 * 2**-24 for the softmax itself.

The action masks the last two use come from the oracles (returned by the replays), never from a device kernel.
"""
from __future__ import annotations

import numpy as np

import sized_ref as SR
from oracle import oracle as O

U = 2.0 ** -24

# The env configs of the replay tests (the step matrix's env_cfg idea): every reward term non-zero and non-dyadic, so
# each term of the fp64 sum is exercised; both reward modes, both bonus modes, the action mask on and off.
TERMS = dict(obs_log2_scale=0.3, base_reward_scale=1.0 / 3.0, empty_tile_reward=-0.07, merge_reward=0.3,
             bonus_scale=0.01, step_reward=-0.003, endgame_penalty=-7.3, invalid_action_penalty=-1.7)
CONFIGS = {
    "R-raw-mask": dict(TERMS, reward_mode="log2", bonus_mode="raw", use_action_mask=True),
    "R-log2-nomask": dict(TERMS, reward_mode="sum", bonus_mode="log2", use_action_mask=False),
    "S-raw-nomask": dict(TERMS, reward_mode="sum", bonus_mode="raw", use_action_mask=False),
    "L-log2-mask": dict(TERMS, reward_mode="log2", bonus_mode="log2", use_action_mask=True),
}


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _flag_map():
    """(oracle bit, device bit) pairs: the B_* -> F_* correspondence tests/test_gpu_step_matrix.py relies on when it
    compares the device's flag byte with the oracle's (the values are equal; F_OVERFLOW has no oracle bit)."""
    from rl2048_amd import _lib as L

    return ((O.B_CHANGED, L.F_CHANGED), (O.B_TERMINATED, L.F_TERMINATED), (O.B_TRUNCATED, L.F_TRUNCATED),
            (O.B_INVALID, L.F_INVALID), (O.B_RESET, L.F_RESET), (O.B_BADACTION, L.F_BADACTION)), L.F_INACTIVE


def _eq(name, got, want, t, lanes):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (name, t, got.shape, want.shape)
    ne = got != want
    if ne.any():
        rows = np.nonzero(ne.reshape(len(got), -1).any(axis=1))[0]
        i = int(rows[0])
        raise AssertionError(f"{name}: row {t}, {len(rows)} episodes differ, first episode {int(lanes[i])}: "
                             f"got {got[i]!r}, oracle {want[i]!r}")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _new_counts():
    return dict(rows=0, terminated=0, truncated=0, invalid=0, changed=0, merges=0, bonus=0)


# ------------------------------------------------------------------------------------------------------------ 4 x 4
def replay_4x4(batch, env_cfg: dict, env_seeds) -> dict:
    """Every episode of a 4 x 4 batch through oracle.EnvBatch.  Returns the counts of terminated, truncated, invalid
    and changed rows, of rows with a merge and of bonus updates (max_tile_seen grew), the rows compared, and under
    "masks" the oracle's action mask of every row's board ([T, n] uint8, bit a = action a; 0 past an episode's end),
    or None when the config has no action mask (nothing then reads one)."""
    fmap, f_inactive = _flag_map()
    boards = _np(batch.boards).view(np.uint64)
    actions, rewards, flags = _np(batch.actions), _np(batch.rewards), _np(batch.flags)
    lengths = _np(batch.lengths).astype(np.int64)
    T, n = actions.shape
    assert boards.shape == rewards.shape == flags.shape == (T, n) and lengths.shape == (n,)
    assert int(lengths.min()) >= 1 and int(lengths.max()) == T, (int(lengths.min()), int(lengths.max()), T)
    ref = O.EnvBatch(n, outputs=["reward", "flags", "prev_board", "board", "max_tile_seen", "active", "unrepresentable",
                                 "mask", "n_merged"], **env_cfg)
    st = ref.reset(np.asarray(env_seeds).astype(np.uint64))
    mask_now, seen = st["mask"].copy(), st["max_tile_seen"].copy()
    masks = np.zeros((T, n), dtype=np.uint8)
    total = np.zeros(n, dtype=np.float64)
    c = _new_counts()
    for t in range(T):
        live = t < lengths
        idx = np.nonzero(live)[0]
        masks[t, idx] = mask_now[idx]
        out = ref.step(np.where(live, actions[t], 255).astype(np.uint8))
        assert int(out["unrepresentable"].sum()) == 0, t
        fl = out["flags"][idx]
        # a lane the oracle skipped has ended there before row t (or the recorded action is not a move)
        _eq("oracle stepped the lane", fl & (O.B_INACTIVE | O.B_BADACTION), np.zeros_like(fl), t, idx)
        _eq("boards", boards[t, idx], out["prev_board"][idx], t, idx)
        _eq("rewards (fp64 bits)", _bits(rewards[t, idx]), _bits(out["reward"][idx]), t, idx)
        want = np.zeros_like(fl)
        for b_bit, f_bit in fmap:
            want |= np.where((fl & b_bit) != 0, f_bit, 0).astype(np.uint8)
        _eq("flags", flags[t, idx] & ~np.uint8(f_inactive), want, t, idx)       # F_OVERFLOW must be clear
        ended = (fl & (O.B_TERMINATED | O.B_TRUNCATED)) != 0
        _eq("episode ends at row lengths - 1 and no earlier", ended, t == lengths[idx] - 1, t, idx)
        total[idx] += out["reward"][idx]                                        # step order, fp64
        c["rows"] += len(idx)
        c["terminated"] += int(((fl & O.B_TERMINATED) != 0).sum())
        c["truncated"] += int(((fl & O.B_TRUNCATED) != 0).sum())
        c["invalid"] += int(((fl & O.B_INVALID) != 0).sum())
        c["changed"] += int(((fl & O.B_CHANGED) != 0).sum())
        c["merges"] += int((out["n_merged"][idx] > 0).sum())
        c["bonus"] += int((out["max_tile_seen"][idx] > seen[idx]).sum())
        seen[idx] = out["max_tile_seen"][idx]
        mask_now = out["mask"].copy()
    st = ref.state()
    every = np.arange(n)
    assert int(st["unrepresentable"].sum()) == 0 and int(st["active"].sum()) == 0
    assert c["rows"] == int(lengths.sum())
    _eq("total_reward (fp64 bits)", _bits(_np(batch.total_reward)), _bits(total), "end", every)
    _eq("max_tile", _np(batch.max_tile).astype(np.int64), st["max_tile_seen"], "end", every)
    _eq("final_boards", _np(batch.final_boards).view(np.uint64), st["board"], "end", every)
    c["masks"] = masks if env_cfg.get("use_action_mask", True) else None
    return c


# ------------------------------------------------------------------------------------------------------- sizes 2..8
def replay_sized(batch, size: int, env_cfg: dict, env_seeds) -> dict:
    """replay_4x4 for a [W, T, n] batch of board size `size`, per episode in SizedRef(size, env_cfg)."""
    from rl2048_amd import _lib as L

    boards = SR.unpack_planes(_np(batch.boards), size)                          # [T, n, N*N] exponents
    final = SR.unpack_planes(_np(batch.final_boards), size)                     # [n, N*N]
    actions, rewards, flags = _np(batch.actions), _np(batch.rewards), _np(batch.flags)
    lengths = _np(batch.lengths).astype(np.int64)
    totals, max_tile = _np(batch.total_reward), _np(batch.max_tile)
    T, n = actions.shape
    assert boards.shape == (T, n, size * size) and rewards.shape == flags.shape == (T, n) and lengths.shape == (n,)
    assert int(lengths.min()) >= 1 and int(lengths.max()) == T, (int(lengths.min()), int(lengths.max()), T)
    masks = np.zeros((T, n), dtype=np.uint8) if env_cfg.get("use_action_mask", True) else None
    c = _new_counts()
    keep = np.uint8(0xFF ^ L.F_INACTIVE)
    for i in range(n):
        e = SR.SizedRef(size, env_cfg)
        e.reset(int(env_seeds[i]))
        total = 0.0
        for t in range(int(lengths[i])):
            where = f"episode {i}, row {t}"
            np.testing.assert_array_equal(boards[t, i], SR.exponents(e.board).reshape(-1), err_msg="boards: " + where)
            if masks is not None:
                masks[t, i] = SR.mask_bits(e.mask())
            seen = e.max_tile_seen
            assert int(actions[t, i]) < 4, where
            r = e.step(int(actions[t, i]))
            assert not r["saturated"], where
            assert _bits(rewards[t, i]) == _bits(r["reward"]), f"rewards: {where}: {rewards[t, i]!r} != {r['reward']!r}"
            want = ((L.F_CHANGED if r["changed"] else 0) | (L.F_TERMINATED if r["terminated"] else 0) |
                    (L.F_TRUNCATED if r["truncated"] else 0) | (L.F_INVALID if r["invalid"] else 0))
            assert int(flags[t, i] & keep) == want, f"flags: {where}: {int(flags[t, i]):#x} != {want:#x}"
            assert (r["terminated"] or r["truncated"]) == (t == lengths[i] - 1), "episode end: " + where
            total += r["reward"]
            c["rows"] += 1
            c["terminated"] += int(r["terminated"])
            c["truncated"] += int(r["truncated"])
            c["invalid"] += int(r["invalid"])
            c["changed"] += int(r["changed"])
            c["merges"] += int(len(r["merged"]) > 0)
            c["bonus"] += int(e.max_tile_seen > seen)
        assert _bits(totals[i]) == _bits(total), f"total_reward: episode {i}: {totals[i]!r} != {total!r}"
        assert int(max_tile[i]) == e.max_tile_seen, f"max_tile: episode {i}: {int(max_tile[i])} != {e.max_tile_seen}"
        np.testing.assert_array_equal(final[i], SR.exponents(e.board).reshape(-1), err_msg=f"final_boards: episode {i}")
    assert c["rows"] == int(lengths.sum())
    c["masks"] = masks
    return c


# ---------------------------------------------------------------------------------------------------------- choices
def choice4(p, u):
    """numpy's Generator.choice(4, p=p) given its one uniform draw u, over rows: p [m, 4] (any float type; numpy
    converts it to fp64 first), cdf = cumsum(p), cdf /= cdf[-1], searchsorted(cdf, u, side="right")."""
    cdf = np.cumsum(np.asarray(p).astype(np.float64), axis=1)
    cdf /= cdf[:, -1:]
    return (cdf <= np.asarray(u, dtype=np.float64)[:, None]).sum(axis=1)


def check_choices(probs, actions, lengths, policy_seeds, greedy: bool, masks) -> int:
    """Every valid row's action from its recorded probabilities.  masks: [T, n] bits from the oracle, or None when the
    env has no action mask.  Returns the number of rows checked."""
    probs, actions = _np(probs), _np(actions)
    lengths = _np(lengths).astype(np.int64)
    T, n = actions.shape
    assert probs.shape == (T, n, 4) and probs.dtype == np.float32
    valid = np.arange(T)[:, None] < lengths[None, :]
    if greedy:
        q = probs if masks is None else probs * ((masks[:, :, None] >> np.arange(4)) & 1).astype(np.float32)
        want = q.argmax(axis=2)                                     # the first maximum
    else:
        u = np.zeros((T, n))
        for i in range(n):
            u[:lengths[i], i] = np.random.default_rng(int(policy_seeds[i])).random(int(lengths[i]))
        want = np.zeros((T, n), dtype=np.int64)
        want[valid] = choice4(probs[valid], u[valid])
    ne = valid & (want != actions)
    if ne.any():
        t, i = (int(x[0]) for x in np.nonzero(ne))
        raise AssertionError(f"choice: {int(ne.sum())} rows differ, first row {t} of episode {i}: action "
                             f"{int(actions[t, i])}, expected {int(want[t, i])} from p = {probs[t, i]!r}")
    assert int(valid.sum()) == int(lengths.sum())
    return int(valid.sum())


# ------------------------------------------------------------------------------------------------------ probabilities
def obs64_sized(e, mode: str, scale: float):
    """test_gpu_deep._obs64 for N x N boards: exponents [m, N*N] (cell k = row-major) -> fp64 obs on the device."""
    import torch
    from test_gpu_deep import DEV

    if mode == "onehot":
        x = np.zeros(e.shape + (17,))
        np.put_along_axis(x, e[:, :, None].astype(np.int64), 1.0, axis=2)
        return torch.from_numpy(x.reshape(len(e), -1)).to(DEV)
    if mode == "log2":
        return torch.from_numpy((e.astype(np.int64) * np.float32(scale)).astype(np.float32).astype(np.float64)).to(DEV)
    return torch.from_numpy(np.where(e > 0, 2.0 ** e.astype(np.float64), 0.0)).to(DEV)


def check_probs(agent, batch, masks, label: str = "", chunk: int = 1 << 16) -> float:
    """Every valid row's recorded probabilities against the fp64 masked softmax of the fp64 forward of the agent's
    parameters on the recorded board: exactly 0.0 where the mask is 0, elsewhere within max_j E_j + 8 * 2**-24, E the
    forward's per-logit fp32 error bound.  (Softmax Jacobian: |dp_k| = p_k |dl_k - sum p_j dl_j| <= max_j |dl_j|; the
    8 u: expf <= 2 ulp, the rounding of l - max x e^-x u <= 0.37 u, three additions and one division, on values
    <= 1.)  masks None: no action mask.  Prints and returns the largest |err| / bound."""
    import torch
    from test_gpu_deep import _fwd64_bound, _obs64

    cfg = agent.env_config
    size = int(getattr(cfg, "size", 4))
    lengths = _np(batch.lengths).astype(np.int64)
    probs = _np(batch.probs)
    T, n = probs.shape[:2]
    valid = np.arange(T)[:, None] < lengths[None, :]
    if size == 4 and _np(batch.boards).ndim == 2:
        b = _np(batch.boards).view(np.uint64)[valid]
        e = ((b[:, None] >> (4 * np.arange(16, dtype=np.uint64))) & np.uint64(15)).astype(np.int64)
        obs = lambda x: _obs64(x, cfg.obs_mode, cfg.obs_log2_scale)
    else:
        e = SR.unpack_planes(_np(batch.boards), size)[valid].astype(np.int64)
        obs = lambda x: obs64_sized(x, cfg.obs_mode, cfg.obs_log2_scale)
    got = probs[valid]
    m = None if masks is None else ((masks[valid][:, None] >> np.arange(4)) & 1).astype(bool)
    W, B = agent.params["W"], agent.params["b"]
    worst = 0.0
    for s in range(0, len(e), chunk):
        z, E = _fwd64_bound(W, B, obs(e[s:s + chunk]), agent.mlp_config.activation)
        g = torch.from_numpy(got[s:s + chunk]).to(z.device).double()
        if m is not None:
            mm = torch.from_numpy(m[s:s + chunk]).to(z.device)
            assert bool(mm.any(dim=1).all()), "a recorded row's board has no valid move"
            z = torch.where(mm, z, torch.full_like(z, -float("inf")))
            assert bool((g[~mm] == 0.0).all()), "a masked action has a non-zero probability"
        p = torch.softmax(z, dim=1)
        if m is not None:
            assert bool((p[~mm] == 0.0).all())
        bound = (E.max(dim=1, keepdim=True).values + 8 * U).expand_as(p)
        ratio = (g - p).abs() / bound
        if m is not None:
            ratio = torch.where(mm, ratio, torch.zeros_like(ratio))
        worst = max(worst, float(ratio.max()))
    assert len(e) == int(lengths.sum())
    print(f"\n{label or cfg.obs_mode}: {len(e)} rows, max |p^ - p| / bound = {worst:.3g}", flush=True)
    assert worst <= 1.0, f"max |p^ - p| / bound = {worst:.3g}"
    return worst
