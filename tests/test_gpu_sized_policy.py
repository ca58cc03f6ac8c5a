"""GPU: g2048_sized_policy (csrc/g2048_sized_policy.hip), the fused forward + action choice for board sizes 2..8,
and the agent's rollout through it (ReinforceAgent.use_fused_sized_policy).

* forward only, every size and obs mode, against an fp64 forward of the reference's encoding (N*N or N*N*17
  features, cell r*N + c, channel e) within the rigorous fp32 bound of tests/test_gpu_deep.py (its helpers are
  imported, not copied);
* size 4 against g2048_deep_policy bit for bit (logits, probabilities, actions, PCG64 streams);
* the choice against g2048_sample on the kernel's own logits and g2048_sized_obs's mask (PCG64 and Philox, greedy,
  compacted lane lists, inactive lanes untouched);
* argument checks;
* the agent with the switch on against the real reference's episodes (tests/golden/sized_agent.npz) and, at the
  other word counts, against an fp64 forward of every recorded step.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_deep import _fwd64, _fwd64_bound, _net

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _lib():
    from rl2048_amd import _lib as L

    L.ensure_device(DEV)
    return L


def _code(L, mode):
    return {"raw": L.OBS_RAW, "log2": L.OBS_LOG2, "onehot": L.OBS_ONEHOT}[mode]


def _planes(e: np.ndarray, size: int, stride: int) -> torch.Tensor:
    """exponents [n, N*N] -> int64 planes [W, stride] (cell k: nibble k & 15 of word k >> 4; lanes >= n are 0)."""
    n = e.shape[0]
    out = np.zeros(((size * size + 15) // 16, stride), dtype=np.uint64)
    for k in range(size * size):
        out[k >> 4, :n] |= e[:, k].astype(np.uint64) << np.uint64(4 * (k & 15))
    return torch.from_numpy(out.view(np.int64)).to(DEV)


def _obs64(e: np.ndarray, mode: str, scale: float) -> torch.Tensor:
    """The reference's encoding of boards of exponents [n, N*N], in fp64 (src/env.py:131-150)."""
    if mode == "onehot":
        x = np.zeros(e.shape + (17,))
        np.put_along_axis(x, e[:, :, None], 1.0, axis=2)
        return torch.from_numpy(x.reshape(len(e), -1)).to(DEV)
    if mode == "log2":
        return torch.from_numpy((e * np.float32(scale)).astype(np.float32).astype(np.float64)).to(DEV)
    return torch.from_numpy(np.where(e > 0, 2.0 ** e, 0.0)).to(DEV)


def _din(mode, size):
    return size * size * (17 if mode == "onehot" else 1)


def _pack(L, size, W, B, code, hidden, dout):
    lib = L.lib()
    harr = (ctypes.c_int32 * len(hidden))(*hidden)
    n = int(lib.g2048_sized_policy_packed_size(size, code, len(hidden), harr))
    assert n > 0
    packed = torch.empty(n, dtype=torch.float32, device=DEV)
    wp = (ctypes.c_void_p * len(W))(*[w.data_ptr() for w in W])
    bp = (ctypes.c_void_p * len(B))(*[b.data_ptr() for b in B])
    L.check(lib.g2048_sized_pack(size, wp, bp, code, len(hidden), harr, dout, L.ptr(packed), n, L.stream_handle(DEV)))
    return packed, harr


def _sparse_boards(rng, n, size, hi=11):
    e = rng.integers(0, hi + 1, size=(n, size * size))
    e[rng.random(e.shape) < 0.35] = 0
    return e


# ---------------------------------------------------------------------------------------------- 1. forward vs fp64
NETS = [("log2", [32], "ReLU"), ("raw", [7], "Sigmoid"), ("onehot", [40, 33, 20, 10], "Sigmoid"),
        ("onehot", [256, 128, 64], "ReLU"), ("onehot", [1], "ReLU")]
FWD_CASES = [(s, m, h, a) for s in range(2, 9) for m, h, a in NETS] + [(8, "log2", [256, 256, 256, 256], "ReLU")]


@pytest.mark.parametrize("dout", [4, 1])
@pytest.mark.parametrize("size,mode,hidden,act", FWD_CASES)
def test_forward_matches_fp64(size, mode, hidden, act, dout):
    """Every output within _fwd64_bound's bound (fan-in = the true row count of W_0) of the fp64 forward."""
    L = _lib()
    code = _code(L, mode)
    rng = np.random.default_rng(1000 * size + len(hidden) * 7 + hidden[0] + dout)
    W, B = _net(rng, _din(mode, size), hidden, dout)
    packed, harr = _pack(L, size, W, B, code, hidden, dout)
    n = 1000 + 17                                         # a ragged last group
    e = rng.integers(0, 16, size=(n, size * size))        # every exponent, the last (partly used) word included
    stride = n + 5
    b = _planes(e, size, stride)
    out = torch.full((n, 4), 7.0, dtype=torch.float32, device=DEV)
    L.check(L.lib().g2048_sized_policy(size, L.ptr(packed), len(hidden), harr,
                                       L.ACT_RELU if act == "ReLU" else L.ACT_SIGMOID, L.ptr(b), stride, None, None,
                                       code, 0.0625, 0, 1, L.RNG_PCG64, None, None, None, 0, None, None, L.ptr(out),
                                       None, n, L.stream_handle(DEV)))
    ref, bound = _fwd64_bound(W, B, _obs64(e, mode, 0.0625), act)
    got = out[:, :dout].double()
    ratio = float(((got - ref).abs() / bound.clamp_min(1e-300)).max())
    print(f"\nN={size} {mode} {hidden} {act} out {dout}: max |err| / bound = {ratio:.3g}")
    assert ratio <= 1.0, ratio
    if dout == 1:
        assert bool((out[:, 1:] == 0).all())


# ------------------------------------------------------------------------------- 2. size 4 == g2048_deep_policy
@pytest.mark.parametrize("mode,hidden", [("log2", [64, 48, 32]), ("onehot", [128, 64])])
def test_size4_equals_deep_policy_bit_for_bit(mode, hidden):
    L = _lib()
    lib, st = L.lib(), L.stream_handle(DEV)
    code = _code(L, mode)
    rng = np.random.default_rng(41 + len(hidden))
    W, B = _net(rng, _din(mode, 4), hidden, 4)
    packed, harr = _pack(L, 4, W, B, code, hidden, 4)
    dsize = int(lib.g2048_deep_packed_size(code, len(hidden), harr))
    dpacked = torch.empty(dsize, dtype=torch.float32, device=DEV)
    wp = (ctypes.c_void_p * len(W))(*[w.data_ptr() for w in W])
    bp = (ctypes.c_void_p * len(B))(*[b.data_ptr() for b in B])
    L.check(lib.g2048_deep_pack(wp, bp, code, len(hidden), harr, 4, L.ptr(dpacked), dsize, st))
    n = 3000 + 17
    b = _planes(_sparse_boards(rng, n, 4, hi=15), 4, n)   # W = 1: the plane is the 4 x 4 bitboard array
    seeds = torch.arange(n, dtype=torch.int64, device=DEV) + 4242
    rs = torch.empty(2 * n, dtype=torch.int64, device=DEV)
    inc = torch.empty(2 * n, dtype=torch.int64, device=DEV)
    buf = torch.empty(n, dtype=torch.int64, device=DEV)
    L.check(lib.g2048_seed_pcg64(L.ptr(seeds), L.ptr(rs), L.ptr(inc), L.ptr(buf), n, st))
    rs2 = rs.clone()
    outs = []
    for sized, state in ((True, rs), (False, rs2)):
        acts = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
        probs = torch.zeros(n, 4, dtype=torch.float32, device=DEV)
        logits = torch.zeros(n, 4, dtype=torch.float32, device=DEV)
        tail = (None, None, code, 0.125, 1, 0, L.RNG_PCG64, L.ptr(state), L.ptr(inc), L.ptr(buf), 0, None,
                L.ptr(probs), L.ptr(logits), L.ptr(acts), n, st)
        if sized:
            L.check(lib.g2048_sized_policy(4, L.ptr(packed), len(hidden), harr, L.ACT_RELU, L.ptr(b), n, *tail))
        else:
            L.check(lib.g2048_deep_policy(L.ptr(dpacked), len(hidden), harr, L.ACT_RELU, L.ptr(b), *tail))
        outs.append((logits, probs, acts))
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    assert torch.equal(rs, rs2) and not torch.equal(rs, torch.zeros_like(rs))
    assert len(torch.unique(outs[0][2])) == 4             # the sampled choice used every action


# --------------------------------------------------------------------------------- 3. the choice == g2048_sample
@pytest.mark.parametrize("rng_name", ["pcg64", "philox"])
@pytest.mark.parametrize("greedy", [0, 1])
@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("size", [5, 8])
def test_choice_equals_g2048_sample(size, compact, greedy, rng_name):
    L = _lib()
    lib, st = L.lib(), L.stream_handle(DEV)
    rng = np.random.default_rng(size * 8 + 4 * compact + 2 * greedy + (rng_name == "philox"))
    hidden = [64, 32]
    W, B = _net(rng, _din("onehot", size), hidden, 4)
    packed, harr = _pack(L, size, W, B, L.OBS_ONEHOT, hidden, 4)
    n = 2000 + 3
    e = _sparse_boards(rng, n, size)
    b = _planes(e, size, n)
    rng_mode = L.RNG_PCG64 if rng_name == "pcg64" else L.RNG_PHILOX
    seeds = torch.arange(n, dtype=torch.int64, device=DEV) + 777
    rs = torch.empty(2 * n, dtype=torch.int64, device=DEV)
    inc = torch.empty(2 * n, dtype=torch.int64, device=DEV)
    buf = torch.empty(n, dtype=torch.int64, device=DEV)
    L.check(lib.g2048_seed_pcg64(L.ptr(seeds), L.ptr(rs), L.ptr(inc), L.ptr(buf), n, st))
    rs0, rs2 = rs.clone(), rs.clone()
    key = 0x1234_5678_9ABC_DEF1
    # lane state: a step count per lane (the Philox counter), ~1 lane in 8 not active
    active = rng.random(n) >= 0.125
    ls_np = rng.integers(0, 500, size=n).astype(np.int64) | np.where(active, L.LS_ACTIVE, 0)
    ls = torch.from_numpy(ls_np.astype(np.int32)).to(DEV)
    idx_np = np.sort(rng.choice(n, size=n // 3, replace=False)).astype(np.int32) if compact else None
    idx = torch.from_numpy(idx_np).to(DEV) if compact else None
    m = n // 3 if compact else n
    acts = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
    probs = torch.full((n, 4), -1.0, dtype=torch.float32, device=DEV)
    logits = torch.full((n, 4), -5.0, dtype=torch.float32, device=DEV)
    L.check(lib.g2048_sized_policy(size, L.ptr(packed), 2, harr, L.ACT_RELU, L.ptr(b), n, L.ptr(ls), L.ptr(idx),
                                   L.OBS_ONEHOT, 1.0, 1, greedy, rng_mode, L.ptr(rs), L.ptr(inc), L.ptr(buf), key,
                                   L.ptr(seeds), L.ptr(probs), L.ptr(logits), L.ptr(acts), m, st))
    # the same choice from the same logits through g2048_sample: only the listed, active lanes are active there
    mask = torch.empty(n, 4, dtype=torch.int8, device=DEV)
    L.check(lib.g2048_sized_obs(size, L.ptr(b), n, L.OBS_NONE, 1.0, None, L.ptr(mask), n, st))
    on = active.copy()
    if compact:
        listed = np.zeros(n, dtype=bool)
        listed[idx_np] = True
        on &= listed
    ls2 = torch.from_numpy(np.where(on, ls_np, ls_np & ~np.int64(L.LS_ACTIVE)).astype(np.int32)).to(DEV)
    acts2 = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
    probs2 = torch.full((n, 4), -1.0, dtype=torch.float32, device=DEV)
    L.check(lib.g2048_sample(L.ptr(logits), L.ptr(mask), L.ptr(ls2), greedy, rng_mode, L.ptr(rs2), L.ptr(inc),
                             L.ptr(buf), key, L.ptr(seeds), L.ptr(probs2), L.ptr(acts2), n, st))
    assert torch.equal(acts, acts2) and torch.equal(probs, probs2)
    assert torch.equal(rs, rs2)
    on_t = torch.from_numpy(on).to(DEV)
    assert bool((acts[on_t] <= 3).all()) and int(on_t.sum()) > n // 4
    if rng_name == "pcg64" and not greedy:
        assert not torch.equal(rs, rs0)
    # lanes outside the index and lanes without LS_ACTIVE keep their sentinels
    assert bool((acts[~on_t] == 9).all()) and bool((probs[~on_t] == -1.0).all()) and bool((logits[~on_t] == -5.0).all())
    # the logits are the forward of the boards; the probabilities the masked softmax of the logits
    ref = _fwd64(W, B, _obs64(e, "onehot", 1.0), "ReLU")[on_t]
    assert float((logits[on_t].double() - ref).abs().max() / ref.abs().max()) < 2e-6
    lg = logits[on_t]
    p_ref = torch.softmax(torch.where(mask[on_t].bool(), lg, torch.full_like(lg, -1e9)).double(), 1)
    assert float((probs[on_t].double() - p_ref).abs().max()) < 1e-6


# ------------------------------------------------------------------------------------------- 4. argument checks
def test_argument_checks():
    L = _lib()
    lib, st = L.lib(), L.stream_handle(DEV)
    rng = np.random.default_rng(3)
    hidden = [16]
    W, B = _net(rng, 25, hidden, 4)
    packed, harr = _pack(L, 5, W, B, L.OBS_LOG2, hidden, 4)
    n = 64
    b = _planes(rng.integers(0, 12, size=(n, 25)), 5, n)
    out = torch.zeros(n, 4, dtype=torch.float32, device=DEV)

    def call(size=5, harr=harr, stride=n, n=n):
        return lib.g2048_sized_policy(size, L.ptr(packed), 1, harr, L.ACT_RELU, L.ptr(b), stride, None, None,
                                      L.OBS_LOG2, 1.0, 0, 1, L.RNG_PCG64, None, None, None, 0, None, None, L.ptr(out),
                                      None, n, st)

    assert call() == L.G2048_OK
    assert call(size=9) == L.G2048_EINVAL
    assert call(size=1) == L.G2048_EINVAL
    assert call(stride=n - 1) == L.G2048_EINVAL
    assert call(harr=(ctypes.c_int32 * 1)(300)) == L.G2048_EINVAL
    assert call(n=(1 << 30) + 1, stride=(1 << 30) + 1) == L.G2048_EINVAL
    assert call(n=0) == L.G2048_OK
    wp = (ctypes.c_void_p * 2)(*[w.data_ptr() for w in W])
    bp = (ctypes.c_void_p * 2)(*[x.data_ptr() for x in B])
    assert lib.g2048_sized_pack(9, wp, bp, L.OBS_LOG2, 1, harr, 4, L.ptr(packed), packed.numel(), st) == L.G2048_EINVAL
    assert lib.g2048_sized_pack(5, wp, bp, L.OBS_LOG2, 1, harr, 4, L.ptr(packed), packed.numel() - 1, st) == \
        L.G2048_EINVAL
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------- 5. agent against the reference
GENERAL = "hipBLASLt forward (active lanes) + g2048_sample + g2048_sized_step per step"


@pytest.mark.parametrize("ci", [0, 1])
def test_agent_rollout_matches_reference(ci):
    """tests/test_gpu_sized_agent.py::test_rollout_matches_reference_run_episode with the fused policy switched on.
    The fixture keeps only seeds whose every draw lies >= 1e-4 from every cdf boundary (recorded minimum 4.2e-4), so
    the 2e-6 agreement of the probabilities cannot flip an action and nothing is skipped."""
    import test_gpu_sized_agent as SA

    D, case = SA.D, SA.CASES[ci]
    n_size, nl = case["env"]["size"], len(case["mlp"]["hidden_sizes"]) + 1
    assert (n_size, case["env"]["obs_mode"], case["mlp"]["hidden_sizes"]) in ((3, "log2", [32]), (5, "onehot", [64, 32]))
    agent = SA._agent(case)
    assert agent.use_fused_sized_policy is False
    agent.use_fused_sized_policy = True
    assert agent._sized_spec() is not None and agent._net_spec() is None and agent._deep_spec() is None
    for u in range(case["updates"]):
        P = f"a{ci}_up{u}_"
        assert (D[P + "margin"] >= 1e-4).all()
        SA._set(agent, SA._before(ci, u, nl, "actor"))
        es, ps = [int(s) for s in D[P + "env_seeds"]], [int(s) for s in D[P + "policy_seeds"]]
        batch = agent.rollout_batch(es, ps, record_probs=True)
        path = agent.last_paths()["rollout"]
        assert "g2048_sized_policy" in path and "g2048_sized_step" in path and "hipBLASLt" not in path
        lens = D[P + "lengths"]
        np.testing.assert_array_equal(batch.lengths.cpu().numpy(), lens)
        boards = SA._exps(batch.boards.cpu().numpy(), n_size)
        acts, rews, probs = batch.actions.cpu().numpy(), batch.rewards.cpu().numpy(), batch.probs.cpu().numpy()
        s = 0
        for i, T in enumerate(lens):
            T = int(T)
            np.testing.assert_array_equal(acts[:T, i], D[P + "actions"][s:s + T], err_msg=f"episode {i}")
            np.testing.assert_array_equal(boards[:T, i], D[P + "boards"][s:s + T])
            np.testing.assert_array_equal(rews[:T, i], D[P + "rewards"][s:s + T])
            np.testing.assert_allclose(probs[:T, i], D[P + "probs"][s:s + T], rtol=0, atol=2e-6)
            s += T
        np.testing.assert_array_equal(batch.total_reward.cpu().numpy(), D[P + "total_reward"])
        np.testing.assert_array_equal(batch.max_tile.cpu().numpy(), D[P + "max_tile"])
    # a changed parameter tensor is re-packed: the rollout differs from the one a stale pack would repeat
    before = batch.probs.clone()
    agent.params["b"][-1] = agent.params["b"][-1] + torch.tensor([2.0, -1.0, 0.5, -2.0], device=DEV)
    agent._params_version += 1
    after = agent.rollout_batch(es, ps, record_probs=True)
    assert "g2048_sized_policy" in agent.last_paths()["rollout"]
    assert not torch.equal(after.probs[0], before[0])
    # ... and with the switch off the general path runs again
    agent.use_fused_sized_policy = False
    agent.rollout_batch(es[:4], ps[:4])
    assert agent.last_paths()["rollout"] == GENERAL


# ------------------------------------------------------------------------- 6. agent at the other word counts
def _make_agent(size, mode, hidden, max_steps=24):
    from rl2048_amd import Game2048EnvConfig
    from rl2048_amd.agent import ReinforceAgent, ReinforceAgentConfig
    from rl2048_amd.mlp import MLPConfig

    cfg = Game2048EnvConfig(size=size, obs_mode=mode, obs_log2_scale=0.125, max_steps=max_steps)
    agent = ReinforceAgent(cfg, MLPConfig(hidden_sizes=hidden, activation="ReLU", init_distribution="HeNormal"),
                           ReinforceAgentConfig(model_seed=size), device=DEV)
    agent.use_fused_sized_policy = True
    return agent


@pytest.mark.parametrize("mode,hidden", [("onehot", [32, 16]), ("log2", [48])])
@pytest.mark.parametrize("size", [2, 6, 7, 8])
def test_agent_rollout_steps_match_fp64(size, mode, hidden):
    from rl2048_amd.vec_env import sized_exponents
    from test_gpu_sized_agent import _mask_of

    agent = _make_agent(size, mode, hidden)
    assert agent._sized_spec() is not None
    n = 64
    batch = agent.rollout_batch(list(range(n)), list(range(500, 500 + n)), record_probs=True)
    assert agent.last_paths()["rollout"] == "g2048_sized_policy + g2048_sized_step per step (active lanes)"
    lens = batch.lengths.cpu().numpy()
    assert (lens >= 1).all() and (lens <= 24).all()
    T = int(lens.max())
    e = sized_exponents(batch.boards, size).reshape(T, n, size * size).cpu().numpy()      # [T, n, N*N]
    valid = np.arange(T)[:, None] < lens[None, :]
    ev = e[valid]                                                                          # [steps, N*N]
    logits = _fwd64([w for w in agent.params["W"]], [b for b in agent.params["b"]], _obs64(ev, mode, 0.125), "ReLU")
    mask = torch.from_numpy(np.stack([_mask_of(x.reshape(size, size)) for x in ev]).astype(bool)).to(DEV)
    assert bool(mask.any(1).all())                     # a recorded step starts from a board with a legal move
    p_ref = torch.softmax(torch.where(mask, logits, torch.full_like(logits, -float("inf"))), 1)
    vt = torch.from_numpy(valid).to(DEV)
    probs = batch.probs[vt].double()
    err = float((probs - p_ref).abs().max())
    print(f"\nN={size} {mode}: {len(ev)} steps, max |p - p64| = {err:.3g}")
    assert err <= 2e-6
    acts = batch.actions[vt].long()
    assert bool(mask.gather(1, acts[:, None]).all())   # every chosen action is legal
    # Philox mode runs the same path
    b2 = agent.rollout_batch(list(range(n)), list(range(900, 900 + n)), rng="philox")
    assert "g2048_sized_policy" in agent.last_paths()["rollout"]
    l2 = b2.lengths.cpu().numpy()
    assert (l2 >= 1).all() and (l2 <= 24).all() and bool(torch.isfinite(b2.total_reward).all())


def test_uncovered_net_falls_back_to_the_general_path():
    agent = _make_agent(6, "log2", [300, 16])
    assert agent._sized_spec() is None
    batch = agent.rollout_batch(list(range(16)), list(range(16, 32)))
    assert agent.last_paths()["rollout"] == GENERAL
    ln = batch.lengths.cpu().numpy()
    assert (ln >= 1).all() and (ln <= 24).all() and bool(torch.isfinite(batch.total_reward).all())
