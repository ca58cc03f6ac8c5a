"""GPU parity of board sizes 2..8 (the g2048_sized_* entry points and the Python layers above them) against
tests/golden/sized.npz, recorded from the real reference by tests/golden/make_golden_sized.py.  Boards, flags, masks,
observations, merged lists, scores and the fp64 reward are compared for equality (the reward with ==).

Lane counts 1, 63 and 257: below a wave, and one past a 256-thread workgroup.  Lane i replays fixture episode i % E.

sized.npz is random play from reset, cut at 60 steps for N >= 5: early-game states only.  Late-game states -- full
and nearly full boards, termination, tiles of 2^8 .. 2^15, saturated merges, a full merged list, the Lemire fallback,
auto-reset after termination -- are in tests/test_gpu_sized_late.py.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from sized_ref import as_sized4 as _as_sized4   # shared with tests/test_gpu_sized_late.py

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SIZES = [2, 3, 5, 6, 7, 8]
LANES = [1, 63, 257]


@pytest.fixture(scope="module")
def lib():
    from rl2048_amd import _lib

    _lib.ensure_device(DEV)
    return _lib


@pytest.fixture(scope="module")
def gold(golden_dir):
    with np.load(os.path.join(golden_dir, "sized.npz")) as z:
        return {k: z[k] for k in z.files}


def words(n):
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
    return np.stack([(p[k >> 4] >> np.uint64(4 * (k & 15))) & np.uint64(15) for k in range(n * n)], axis=-1).astype(np.uint8)


def _cfg(n, kw):
    from rl2048_amd import Game2048EnvConfig

    return Game2048EnvConfig(size=n, **kw)


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("c", [1, 2, 3, 4])
@pytest.mark.parametrize("n", SIZES)
def test_vec_env_matches_reference_episodes(gold, lib, n, c, lanes):
    from rl2048_amd import VecGame2048Env

    kw = json.loads(str(gold["env_cfgs"]))[str(c)]
    p = f"n{n}_c{c}_"
    seeds, starts, lens = gold[p + "ep_seed"], gold[p + "ep_start"].astype(int), gold[p + "ep_len"].astype(int)
    E, T, W, LEN = len(seeds), int(lens.max()), words(n), n * (n // 2)
    ep = np.arange(lanes) % E
    cfg = _cfg(n, kw)
    env = VecGame2048Env(lanes, cfg, device=DEV, record_merged=True)
    envp = VecGame2048Env(lanes, cfg, device=DEV, packed_mask=True)        # the packed action-mask form
    lane_seeds = [int(seeds[e]) for e in ep]
    obs0, _ = env.reset(seed=lane_seeds)
    envp.reset(seed=lane_seeds)
    OW = n * n * (17 if cfg.obs_mode == "onehot" else 1)
    board0 = obs0["board"] if cfg.use_action_mask else obs0
    assert tuple(board0.shape) == ((lanes, n, n, 17) if cfg.obs_mode == "onehot" else (lanes, n, n))
    assert np.array_equal(unpack_planes(env.board.cpu().numpy(), n), gold[p + "reset_board"][ep])
    assert np.array_equal(env.obs.cpu().numpy().reshape(lanes, OW), gold[p + "reset_obs"][ep])
    rm = gold[p + "reset_mask"][ep]
    assert np.array_equal(env.mask.cpu().numpy(), ((rm[:, None] >> np.arange(4)) & 1).astype(np.int8))
    assert np.array_equal(envp.mask_bits.cpu().numpy(), rm)
    assert torch.equal(env.boards_exponents().reshape(lanes, -1).to(torch.uint8).cpu(),
                       torch.from_numpy(gold[p + "reset_board"][ep]))
    # actions per (t, lane); a lane whose episode is over gets action 0 (it reports F_INACTIVE)
    acts = np.zeros((T, lanes), dtype=np.uint8)
    valid = np.zeros((T, lanes), dtype=bool)
    idx = np.zeros((T, lanes), dtype=np.int64)
    for i, e in enumerate(ep):
        acts[:lens[e], i] = gold[p + "action"][starts[e]:starts[e] + lens[e]]
        valid[:lens[e], i] = True
        idx[:lens[e], i] = np.arange(starts[e], starts[e] + lens[e])
    acts_d = torch.from_numpy(acts).to(DEV)
    # step_into with trajectory rows: prev_board row t of a [W, cap, n] tensor (plane stride cap * n != n)
    traj = torch.zeros(W, T, lanes, dtype=torch.int64, device=DEV)
    rew32 = torch.zeros(T, lanes, dtype=torch.float32, device=DEV)
    rew64 = torch.zeros(T, lanes, dtype=torch.float64, device=DEV)
    flags = torch.zeros(T, lanes, dtype=torch.uint8, device=DEV)
    flagsp = torch.zeros(T, lanes, dtype=torch.uint8, device=DEV)
    rec = {k: [] for k in ("board", "obs", "mask", "merged", "state", "score", "boardp", "bits", "obsp")}
    for t in range(T):
        env.step_into(acts_d[t], reward=rew32[t], flags=flags[t], prev_board=traj[:, t], reward64=rew64[t])
        envp.step_into(acts_d[t], flags=flagsp[t])
        rec["board"].append(env.board.clone())
        rec["obs"].append(env.obs.clone())
        rec["mask"].append(env.mask.clone())
        rec["merged"].append(env.merged.clone())
        rec["state"].append(env.state.clone())
        rec["score"].append(env.score.clone())
        rec["boardp"].append(envp.board.clone())
        rec["bits"].append(envp.mask_bits.clone())
        rec["obsp"].append(envp.obs.clone())
    h = {k: torch.stack(v).cpu().numpy() for k, v in rec.items()}
    fl, v = flags.cpu().numpy(), valid
    g = lambda k: gold[p + k][idx]                                       # noqa: E731  [T, lanes, ...]
    assert np.array_equal(unpack_planes(np.moveaxis(h["board"], 1, 0), n)[v], g("board")[v])
    r64 = rew64.cpu().numpy()
    for t, i in zip(*np.nonzero(v)):                                     # the fp64 reward, with ==
        assert r64[t, i] == gold[p + "reward"][idx[t, i]], (n, c, t, i)
    assert np.array_equal(rew32.cpu().numpy()[v], g("reward").astype(np.float32)[v])
    assert np.array_equal(((fl & 2) != 0)[v], g("terminated")[v])
    assert np.array_equal(((fl & 4) != 0)[v], g("truncated")[v])
    assert np.array_equal(((fl & 8) != 0)[v], g("invalid")[v])
    assert (fl[~v] == lib.F_INACTIVE).all() and not (fl[v] & (lib.F_INACTIVE | lib.F_BADACTION | lib.F_RESET)).any()
    st = h["state"].view(np.uint32)
    assert np.array_equal((np.int64(1) << ((st >> 20) & 31).astype(np.int64))[v], g("max_tile_seen")[v])
    assert np.array_equal((st & 0xFFFFF).astype(np.int64)[v], g("step_index")[v])
    assert np.array_equal(h["score"][v], g("score")[v])
    gm = g("mask")
    assert np.array_equal(h["mask"][v], ((gm[..., None] >> np.arange(4)) & 1).astype(np.int8)[v])
    assert np.array_equal(h["bits"][v], gm[v])
    assert np.array_equal(h["obs"].reshape(T, lanes, OW)[v], g("obs")[v])
    assert np.array_equal(h["obsp"].reshape(T, lanes, OW)[v], g("obs")[v])
    assert np.array_equal(h["merged"][v], g("merged")[v]) and h["merged"].shape == (T, lanes, LEN)
    assert np.array_equal(h["boardp"], h["board"]) and np.array_equal(flagsp.cpu().numpy(), fl)
    # prev_board rows: the board before step t
    prev = unpack_planes(traj.cpu().numpy(), n)                          # [T, lanes, N*N]
    want_prev = np.concatenate([gold[p + "reset_board"][ep][None], g("board")[:-1]])
    pv = v.copy()
    pv[1:] &= v[:-1]
    assert np.array_equal(prev[pv], want_prev[pv])



@pytest.mark.parametrize("rng,c", [("pcg64", 2), ("philox", 3), ("pcg64", 1)])
def test_sized_step_at_size_4_equals_step(gold, lib, rng, c):
    """g2048_sized_step(size=4) against g2048_step: 300 steps of random actions, 257 lanes, auto-reset on; every
    output and every piece of lane state, bit for bit."""
    from rl2048_amd import VecGame2048Env
    from rl2048_amd.vec_env import decode_merged, decode_merged_sized

    kw = dict(json.loads(str(gold["env_cfgs"]))[str(c)])
    if kw.get("max_steps") is None:
        kw["max_steps"] = 90
    n = 257
    mk = lambda: VecGame2048Env(n, _cfg(4, kw), device=DEV, rng=rng, auto_reset=True, reset_stride=1000,  # noqa: E731
                                record_merged=True, record_prev_board=True, record_reward64=True)
    a, b = mk(), _as_sized4(mk(), lib)
    a.reset(seed=77)
    b.reset(seed=77)
    assert torch.equal(a.board, b.board[0]) and torch.equal(a.obs, b.obs) and torch.equal(a.mask, b.mask)
    g = torch.Generator(device="cpu").manual_seed(5)
    acts = torch.randint(0, 4, (300, n), generator=g, dtype=torch.uint8).to(DEV)
    ok = torch.ones((), dtype=torch.bool, device=DEV)
    nres = torch.zeros((), dtype=torch.int64, device=DEV)
    for t in range(300):
        a.step_into(acts[t])
        b.step_into(acts[t])
        for x, y in ((a.board, b.board[0]), (a.prev_board, b.prev_board[0]), (a.state, b.state), (a.seed, b.seed),
                     (a.reward, b.reward), (a.reward64, b.reward64), (a.flags, b.flags), (a.mask, b.mask),
                     (a.obs, b.obs), (a._score_add, b._score_add), (a.score, b.score)):
            ok &= (x == y).all()
        if rng == "pcg64":
            ok &= (a.rng_state == b.rng_state).all() & (a.rng_inc == b.rng_inc).all() & (a.rng_uint == b.rng_uint).all()
        if t % 25 == 0:   # merged lists: nibbles e - 1 in a word against bytes e
            ma, mb = a.merged.cpu().numpy(), b.merged.cpu().numpy()
            assert all(decode_merged(int(x)) == decode_merged_sized(y) for x, y in zip(ma, mb)), t
        nres += ((b.flags & lib.F_RESET) != 0).sum()
    assert bool(ok)
    assert int(nres) > 0                          # lanes did auto-reset


@pytest.mark.parametrize("n", [3, 8])
def test_philox_spawn_and_auto_reset(lib, n):
    from rl2048_amd import Game2048EnvConfig, VecGame2048Env

    lanes, stride, W = 257, 1000, words(n)
    env = VecGame2048Env(lanes, Game2048EnvConfig(size=n, obs_mode="log2", reward_mode="log2", max_steps=12), device=DEV,
                         rng="philox", auto_reset=True, reset_stride=stride, record_prev_board=True)
    env.reset(seed=5)
    g = torch.Generator(device="cpu").manual_seed(n)
    acts = torch.randint(0, 4, (30, lanes), generator=g, dtype=torch.uint8).to(DEV)
    moved = torch.zeros(W, lanes, dtype=torch.int64, device=DEV)
    mflags = torch.zeros(lanes, dtype=torch.uint8, device=DEV)
    seen_reset = 0
    for t in range(30):
        seed_before = env.seed.clone()
        env.step_into(acts[t])
        lib.check(lib.lib().g2048_sized_move(n, env.prev_board.data_ptr(), lanes, acts[t].data_ptr(), moved.data_ptr(),
                                             lanes, None, mflags.data_ptr(), lanes, lib.stream_handle(DEV)))
        fl = env.flags.cpu().numpy()
        pre, post = unpack_planes(moved.cpu().numpy(), n), unpack_planes(env.board.cpu().numpy(), n)
        prev = unpack_planes(env.prev_board.cpu().numpy(), n)
        changed, reset = (fl & lib.F_CHANGED) != 0, (fl & lib.F_RESET) != 0
        assert np.array_equal(changed, (mflags.cpu().numpy() & lib.F_CHANGED) != 0)
        live = changed & ~reset
        d = post[live] != pre[live]
        assert (d.sum(axis=1) == 1).all()                                 # exactly one new tile ...
        assert (pre[live][d] == 0).all() and np.isin(post[live][d], (1, 2)).all()   # ... a 2 or 4 in an empty cell
        still = ~changed & ~reset
        assert np.array_equal(post[still], prev[still])
        # auto-reset reseeds by reset_stride and starts a fresh two-tile episode
        sd = env.seed.cpu().numpy()
        assert np.array_equal(sd[reset], seed_before.cpu().numpy()[reset] + stride)
        assert np.array_equal(sd[~reset], seed_before.cpu().numpy()[~reset])
        assert ((post[reset] != 0).sum(axis=1) == 2).all() and np.isin(post[reset], (0, 1, 2)).all()
        assert (env.step_count.cpu().numpy()[reset] == 0).all()
        seen_reset += int(reset.sum())
    assert seen_reset >= lanes                                            # max_steps 12 within 30 steps


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("n", [3, 5])
def test_obs_and_symmetries_match_reference(gold, lib, n, lanes):
    W = words(n)
    for k, (mode, scale) in enumerate(json.loads(str(gold["sym_kinds"]))):
        p = f"n{n}_s{k}_"
        sel = np.arange(lanes) % len(gold[p + "board_in"])
        boards = torch.from_numpy(pack_planes(gold[p + "board_in"][sel], n)).to(DEV)
        acts = torch.from_numpy(gold[p + "action_in"][sel]).to(DEV)
        ob = torch.zeros(W, 8 * lanes + 3, dtype=torch.int64, device=DEV)       # out_stride = 8 lanes + 3
        oa = torch.zeros(8 * lanes, dtype=torch.uint8, device=DEV)
        lib.check(lib.lib().g2048_sized_symmetries(n, boards.data_ptr(), lanes, acts.data_ptr(), ob.data_ptr(),
                                                   8 * lanes + 3, oa.data_ptr(), lanes, lib.stream_handle(DEV)))
        OW = n * n * (17 if mode == "onehot" else 1)
        obs = torch.zeros(8 * lanes, OW, dtype=torch.float32, device=DEV)
        mask = torch.zeros(8 * lanes, 4, dtype=torch.int8, device=DEV)
        lib.check(lib.lib().g2048_sized_obs(n, ob.data_ptr(), 8 * lanes + 3, {"log2": 1, "onehot": 2}[mode], scale,
                                            obs.data_ptr(), mask.data_ptr(), 8 * lanes, lib.stream_handle(DEV)))
        assert np.array_equal(obs.cpu().numpy().reshape(8, lanes, OW), np.moveaxis(gold[p + "obs_out"][sel], 1, 0))
        assert np.array_equal(mask.cpu().numpy().reshape(8, lanes, 4), np.moveaxis(gold[p + "mask_out"][sel], 1, 0))
        assert np.array_equal(oa.cpu().numpy().reshape(8, lanes), gold[p + "action_out"][sel].T)
        assert not ob[:, 8 * lanes:].any()                                       # nothing past the planes' lanes


@pytest.mark.parametrize("n", [3, 5])
def test_drop_ins_match_reference_episodes(gold, lib, n):
    from rl2048_amd.env import Game2048, Game2048Env

    cfgs = json.loads(str(gold["env_cfgs"]))
    for c in ("1", "3"):
        p = f"n{n}_c{c}_"
        cfg = _cfg(n, cfgs[c])
        env = Game2048Env(cfg, device=DEV)
        shape = (n, n, 17) if cfg.obs_mode == "onehot" else (n, n)
        space = env.observation_space["board"] if cfg.use_action_mask else env.observation_space
        assert space.shape == shape
        e = 1
        s0, ln = int(gold[p + "ep_start"][e]), int(gold[p + "ep_len"][e])
        obs, info = env.reset(seed=int(gold[p + "ep_seed"][e]))
        board = obs["board"] if cfg.use_action_mask else obs
        assert board.shape == shape and np.array_equal(board.reshape(-1), gold[p + "reset_obs"][e])
        vals = lambda ex: np.where(ex > 0, np.int64(1) << ex.astype(np.int64), 0).reshape(n, n).tolist()  # noqa: E731
        assert info["raw_state"] == vals(gold[p + "reset_board"][e]) and env.state == info["raw_state"]
        for t in range(ln):
            j = s0 + t
            obs, r, term, trunc, info = env.step(int(gold[p + "action"][j]))
            board = obs["board"] if cfg.use_action_mask else obs
            assert np.array_equal(board.reshape(-1), gold[p + "obs"][j])
            if cfg.use_action_mask:
                assert [int(x) for x in obs["action_mask"]] == [(int(gold[p + "mask"][j]) >> a) & 1 for a in range(4)]
            assert isinstance(r, float) and r == gold[p + "reward"][j]
            assert term == bool(gold[p + "terminated"][j]) and trunc == bool(gold[p + "truncated"][j])
            assert info["merged"] == [1 << int(x) for x in gold[p + "merged"][j] if x]
            assert isinstance(info["merged"], list)
            assert info["score"] == int(gold[p + "score"][j]) and info["raw_state"] == vals(gold[p + "board"][j])
            assert info["invalid_action"] == bool(gold[p + "invalid"][j]) and info["step_index"] == t + 1
            assert env.max_tile_seen == int(gold[p + "max_tile_seen"][j])
        assert env.render(mode="ansi").count("\n") == 2 * n
    # Game2048(size): the same spawn stream and moves without the env around it
    p = f"n{n}_c1_"
    game = Game2048(size=n, device=DEV)
    assert game.reset(seed=int(gold[p + "ep_seed"][0])) == vals(gold[p + "reset_board"][0])
    prev = gold[p + "reset_board"][0]
    for t in range(int(gold[p + "ep_len"][0])):
        j = int(gold[p + "ep_start"][0]) + t
        changed, state, merged, done = game.step(int(gold[p + "action"][j]))
        assert state == vals(gold[p + "board"][j]) and changed == bool((prev != gold[p + "board"][j]).any())
        assert merged == [1 << int(x) for x in gold[p + "merged"][j] if x] and done == bool(gold[p + "terminated"][j])
        assert game.score == int(gold[p + "score"][j])
        assert game.get_action_mask() == [(int(gold[p + "mask"][j]) >> a) & 1 for a in range(4)]
        prev = gold[p + "board"][j]


def test_error_paths(lib):
    from rl2048_amd import Game2048EnvConfig, VecGame2048Env
    from rl2048_amd.env import Game2048

    for bad in (1, 9):
        with pytest.raises(ValueError):
            VecGame2048Env(4, Game2048EnvConfig(size=bad), device=DEV)
        with pytest.raises(ValueError):
            Game2048(size=bad, device=DEV)
        assert lib.lib().g2048_sized_words(bad) == -1
    assert [lib.lib().g2048_sized_words(s) for s in range(2, 9)] == [1, 1, 1, 2, 3, 4, 4]
    n = 64
    boards = torch.zeros(2, n, dtype=torch.int64, device=DEV)
    obs = torch.zeros(n, 25, dtype=torch.float32, device=DEV)
    s = lib.stream_handle(DEV)
    assert lib.lib().g2048_sized_obs(9, boards.data_ptr(), n, 1, 1.0, obs.data_ptr(), None, n, s) == lib.G2048_EINVAL
    assert lib.lib().g2048_sized_obs(5, boards.data_ptr(), n - 1, 1, 1.0, obs.data_ptr(), None, n, s) == lib.G2048_EINVAL
    assert b"plane_stride" in lib.lib().g2048_last_error()
    with pytest.raises(ValueError):
        lib.check(lib.lib().g2048_sized_obs(5, boards.data_ptr(), n - 1, 1, 1.0, obs.data_ptr(), None, n, s))
    env = VecGame2048Env(n, Game2048EnvConfig(size=5), device=DEV)
    env.reset(seed=1)
    acts = torch.zeros(n, dtype=torch.uint8, device=DEV)
    out = env._sized_out(env.reward, env.flags, torch.zeros(2, n, dtype=torch.int64, device=DEV), True, None)
    out.prev_stride = n - 1                                               # a prev_board stride below n
    rc = lib.lib().g2048_sized_step(5, ctypes.byref(env._lanes), n, acts.data_ptr(), ctypes.byref(env._cfg),
                                    ctypes.byref(out), env.rng_mode, 0, 0, 0, n, s)
    assert rc == lib.G2048_EINVAL
    with pytest.raises(ValueError):
        env.step_into(acts, prev_board=torch.zeros(n, 2, dtype=torch.int64, device=DEV).t()[:, :n])  # planes not contiguous
    assert lib.lib().g2048_sized_obs(5, boards.data_ptr(), n, 1, 1.0, obs.data_ptr(), None, n, s) == lib.G2048_OK
    torch.cuda.synchronize()
