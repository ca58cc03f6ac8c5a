"""GPU: the fused gradient for board sizes 2..8 (g2048_sized_grad + g2048_sized_onehot_dw1, include/g2048_sized.h) and
the agent path behind ReinforceAgent.use_fused_sized_grad.

Kernel level: direct C calls on random boards (exponents 0..15 in every cell, so full boards and high tiles occur)
with random fp32 nets, coefficients, actions and targets, against an fp64 torch evaluation (EG.fwd64_deep /
EG.bwd64_deep) on g2048_sized_obs features, which tests/test_gpu_sized.py pins bit-exactly to the reference.
  * Sigmoid: every folded tensor within 1e-5 normwise of plain fp64 (the project's gradient bar,
    RF.assert_grad_parity).
  * ReLU: within 1e-5 of fp64 under the kernel's own activation pattern (hidden_out[l] > 0), and that pattern is held
    against fp64's own by EG.pattern_flip_check_deep's rigorous fp32 bound: zero violations.
  * value_out / delta_out: inside the rigorous forward-error bound _fwd64_bound (restated from tests/test_gpu_deep.py).
    d0_out is a backward value (layer 0's deltas), which a forward bound does not cover: it is held to the gradient
    bar, 1e-5 normwise of fp64 under the same pattern.
  * Every output buffer carries a sentinel tail and the board planes sentinel lanes between n and plane_stride, all
    asserted intact after the call: an out-of-bounds store shows without a fault.
Raw obs reach 2^15, so the raw nets' first layer is scaled by 2^-12: with O(1) weights the logits are O(1e5), their
fp32 rounding is O(1e-2) absolute, and a softmax that is not saturated then differs by 1 % for reasons that have nothing
to do with the kernel.
Agent level: update_from_batch with the switch on, on the agent's own rollouts and on the reference's recorded
batches (tests/golden/sized_agent.npz), against an fp64 evaluation of update_batch's formula built here from the EG
pieces."""
import ctypes
import json

import numpy as np
import pytest
import torch

import exact_grad as EG
import ref_fixtures as RF
from sized_grad_ref import (BAR, DEV, SCALE, Run, _boards, _exact_update, _features, _fwd64_bound, _guarded, _intact,
                            _lib, _loss_grad, _mode, _net, _pack, _r32, _words)
from test_gpu_ref_fixtures import assert_step_matches

pytestmark = pytest.mark.gpu


def _check_case(size, mode, hidden, act, n=217, nparts=2, stride_extra=0, seed=0, variants=("actor", "mse", "huber")):
    L = _lib()
    rng = np.random.default_rng(1000 * size + 10 * len(hidden) + hidden[0] + seed)
    cells = size * size
    din = cells * (17 if mode == "onehot" else 1)
    e, planes = _boards(rng, n, size, n + stride_extra)
    x, mk = _features(L, size, planes, n, mode, SCALE)
    t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    for var in variants:
        critic = var != "actor"
        dout = 1 if critic else 4
        W, B = _net(rng, din, hidden, dout, 2.0 ** -12 if mode == "raw" else 1.0)
        actions = t(rng.integers(0, 4, n, dtype=np.uint8))
        coef = t(rng.standard_normal(n).astype(np.float32))
        target = t(rng.standard_normal(n).astype(np.float32))
        hd = 0.5
        loss = 1 if var == "huber" else 0
        r = Run(L, size, mode, hidden, act, W, B, planes, n, critic, loss, hd, None if critic else actions, coef,
                target if critic else None, nparts)
        W64, B64 = [w.double() for w in W], [b.double() for b in B]
        masks = [h > 0 for h in r.hidden] if act == "ReLU" else None
        zs, acts, out = EG.fwd64_deep(W64, B64, x, act, masks)
        if act == "ReLU":
            stats = {}
            EG.pattern_flip_check_deep(W64, B64, x, EG.fwd64_deep(W64, B64, x, act)[0], masks, stats, "k")
            assert sum(stats["k"]["viol"]) == 0, stats
        else:   # the activations the kernel reports are its forward's: inside the forward bound of layer 0
            assert float((r.hidden[0].double() - acts[1]).abs().max()) < 1e-5
        g = _loss_grad(critic, loss, hd, out, mk, actions, coef, target)
        ref = [torch.zeros_like(p) for p in W64 + B64]
        EG.bwd64_deep(W64, zs, acts, g, ref, act)
        errs = {j: EG._rel(a, b) for j, (a, b) in enumerate(zip(r.grads, ref))}
        print(f"\nN={size} {mode} {hidden} {act} {var}: max normwise error {max(errs.values()):.3g}")
        assert max(errs.values()) < BAR, errs
        if critic:
            z, Ez = _fwd64_bound(W, B, x, act)
            v = r.value.double()
            assert bool(((v - z[:, 0]).abs() <= Ez[:, 0]).all())
            dl = target.double() - z[:, 0]
            assert bool(((r.delta.double() - dl).abs() <= Ez[:, 0] + 2.0 ** -23 * dl.abs()).all())
            assert torch.equal(r.delta, target - r.value)   # delta_out = target - V on the kernel's own V
        if mode == "onehot":
            # delta_0 in fp64 under the same pattern
            L1 = len(W64)
            d = g
            for l in range(L1 - 1, 0, -1):
                dh = d @ W64[l].t()
                d = dh * ((zs[l - 1] > 0).double() if act == "ReLU" else acts[l] * (1.0 - acts[l]))
            assert EG._rel(r.d0[:, :hidden[0]], d) < BAR
            assert bool((r.d0[:, hidden[0]:] == 0).all())
    return True


LOG2_NETS = [([48], "ReLU"), ([64, 48, 32], "ReLU"), ([40, 33, 20, 10], "Sigmoid")]
ONEHOT_NETS = [([32, 16], "Sigmoid"), ([128, 64], "ReLU")]
CASES = ([(N, "log2", h, a) for N in range(2, 9) for h, a in LOG2_NETS] +
         [(N, "onehot", h, a) for N in range(2, 9) for h, a in ONEHOT_NETS] +
         [(N, "raw", h, a) for N in (3, 8) for h, a in LOG2_NETS[1:]] +
         [(N, "onehot", [256, 128, 64], "ReLU") for N in (3, 8)] + [(N, "log2", [256, 128], "ReLU") for N in (3, 8)])


@pytest.mark.parametrize("size,mode,hidden,act", CASES,
                         ids=[f"N{N}-{m}-{'x'.join(map(str, h))}-{a}" for N, m, h, a in CASES])
def test_kernel_matches_fp64(size, mode, hidden, act):
    """n = 217 samples on 2 workgroups: several groups each and a ragged last one; actor, critic MSE and critic Huber."""
    _check_case(size, mode, hidden, act)


@pytest.mark.parametrize("n", [1, 31, 32, 33])
@pytest.mark.parametrize("size,mode,hidden,act", [(5, "log2", [48, 40], "ReLU"), (6, "onehot", [40, 24], "Sigmoid"),
                                                  (8, "raw", [33], "ReLU")])
def test_edges_small_n_idle_workgroups_and_wide_stride(size, mode, hidden, act, n):
    """n around one group, more workgroups than groups (their slabs exactly zero), plane_stride > n."""
    _check_case(size, mode, hidden, act, n=n, nparts=5, stride_extra=11, seed=n, variants=("actor", "huber"))
    L = _lib()
    rng = np.random.default_rng(n)
    din = size * size * (17 if mode == "onehot" else 1)
    e, planes = _boards(rng, n, size, n + 3)
    W, B = _net(rng, din, hidden, 4, 2.0 ** -12 if mode == "raw" else 1.0)
    t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    r = Run(L, size, mode, hidden, act, W, B, planes, n, False, actions=t(rng.integers(0, 4, n, dtype=np.uint8)),
            coef=t(rng.standard_normal(n).astype(np.float32)), nparts=5)
    groups = -(-n // 32)
    assert bool((r.part[groups:] == 0).all()), "an idle workgroup's slab must be exactly zero"
    assert bool((r.part[:groups] != 0).any())


def test_two_identical_calls_give_equal_slabs():
    L = _lib()
    rng = np.random.default_rng(77)
    t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    for size, mode, hidden, act in ((7, "onehot", [128, 64], "ReLU"), (6, "log2", [64, 48, 32], "Sigmoid")):
        n = 1000 + 13
        din = size * size * (17 if mode == "onehot" else 1)
        e, planes = _boards(rng, n, size)
        W, B = _net(rng, din, hidden, 4)
        actions, coef = t(rng.integers(0, 4, n, dtype=np.uint8)), t(rng.standard_normal(n).astype(np.float32))
        packs = _pack(L, size, W, B, mode, hidden, 4)
        a = Run(L, size, mode, hidden, act, W, B, planes, n, False, actions=actions, coef=coef, nparts=7, packs=packs)
        b = Run(L, size, mode, hidden, act, W, B, planes, n, False, actions=actions, coef=coef, nparts=7, packs=packs)
        assert torch.equal(a.part, b.part) and torch.equal(a.d0, b.d0)
        assert all(torch.equal(x, y) for x, y in zip(a.grads, b.grads))
        assert all(torch.equal(x, y) for x, y in zip(a.hidden, b.hidden))
        # and without hidden_out: it is a guarded store that changes nothing else
        c = Run(L, size, mode, hidden, act, W, B, planes, n, False, actions=actions, coef=coef, nparts=7, packs=packs,
                want_hidden=False)
        assert torch.equal(a.part, c.part) and torch.equal(a.d0, c.d0)


@pytest.mark.parametrize("mode,hidden,act", [("log2", [64, 48, 32], "ReLU"), ("onehot", [128, 64], "Sigmoid"),
                                             ("raw", [40], "Sigmoid")])
def test_size_4_agrees_with_g2048_deep_grad(mode, hidden, act):
    """N = 4 through the sized entry against the 4 x 4 kernel on the same single-word boards: within 1e-5 normwise (not
    bit for bit: the 4 x 4 kernel runs other instantiations -- a k-split dense forward, 64-sample groups)."""
    from rl2048_amd.agent import ReinforceAgent

    L = _lib()
    lib, st = L.lib(), L.stream_handle(DEV)
    rng = np.random.default_rng(44)
    n, nparts = 500 + 7, 3
    din = 16 * (17 if mode == "onehot" else 1)
    e, planes = _boards(rng, n, 4)
    W, B = _net(rng, din, hidden, 4, 2.0 ** -12 if mode == "raw" else 1.0)
    t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    actions, coef = t(rng.integers(0, 4, n, dtype=np.uint8)), t(rng.standard_normal(n).astype(np.float32))
    r = Run(L, 4, mode, hidden, act, W, B, planes, n, False, actions=actions, coef=coef, nparts=nparts)
    nh, code = len(hidden), _mode(L, mode)
    harr = (ctypes.c_int32 * nh)(*hidden)
    sz = int(lib.g2048_deep_packed_size(code, nh, harr))
    packed = torch.empty(sz, dtype=torch.float32, device=DEV)
    wp = (ctypes.c_void_p * len(W))(*[w.data_ptr() for w in W])
    bp = (ctypes.c_void_p * len(B))(*[b.data_ptr() for b in B])
    L.check(lib.g2048_deep_pack(wp, bp, code, nh, harr, 4, L.ptr(packed), sz, st))
    gsz = int(lib.g2048_deep_grad_pack_size(code, nh, harr))
    gpacked = torch.empty(gsz, dtype=torch.float32, device=DEV)
    L.check(lib.g2048_deep_grad_pack(wp, code, nh, harr, L.ptr(gpacked), gsz, st))
    slab = int(lib.g2048_deep_grad_slab(code, nh, harr))
    part = torch.empty(nparts, slab, dtype=torch.float32, device=DEV)
    Hp = [_r32(h) for h in hidden]
    d0 = torch.empty(n, Hp[0], dtype=torch.float32, device=DEV)
    b1 = planes[0].contiguous()
    act_code = {"ReLU": L.ACT_RELU, "Sigmoid": L.ACT_SIGMOID}[act]
    L.check(lib.g2048_deep_grad(L.ptr(packed), L.ptr(gpacked), nh, harr, act_code, code, SCALE, 1, L.ptr(b1),
                                L.ptr(actions), L.ptr(coef), 0, 0, 1.0, None, None, None,
                                L.ptr(d0) if mode == "onehot" else None, n, L.ptr(part), nparts, None, st))
    acc = torch.zeros(slab, dtype=torch.float64, device=DEV)
    L.check(lib.g2048_fold_partials(L.ptr(part), nparts, slab, L.ptr(acc), st))
    pw, pb = ReinforceAgent._deep_slab_layout(hidden, mode == "onehot")
    ref = []
    if mode == "onehot":
        assert EG._rel(r.d0, d0) < BAR
    else:
        ref.append((r.grads[0], acc[pw[0]:pw[0] + 16 * Hp[0]].view(16, Hp[0])[:, :hidden[0]]))
    for l in range(1, nh):
        ref.append((r.grads[l], acc[pw[l]:pw[l] + Hp[l - 1] * Hp[l]].view(Hp[l - 1], Hp[l])[:hidden[l - 1], :hidden[l]]))
    ref.append((r.grads[nh], acc[pw[nh]:pw[nh] + Hp[-1] * 4].view(Hp[-1], 4)[:hidden[-1]]))
    for l in range(nh):
        ref.append((r.grads[nh + 1 + l], acc[pb[l]:pb[l] + Hp[l]][:hidden[l]]))
    ref.append((r.grads[2 * nh + 1], acc[pb[nh]:pb[nh] + 4]))
    for got, want in ref:
        assert EG._rel(got, want) < BAR


@pytest.mark.parametrize("size", [2, 5, 8])
@pytest.mark.parametrize("h1,m,per", [(64, 3, 1024), (100, 5000, 777), (256, 3000, 512), (1, 999, 100), (200, 33, 16)])
def test_sized_onehot_dw1_matches_fp64(size, h1, m, per):
    L = _lib()
    lib, st = L.lib(), L.stream_handle(DEV)
    rng = np.random.default_rng(h1 + m + size)
    cells = size * size
    e, planes = _boards(rng, m, size, m + 5)
    before = planes.clone()
    ld = h1 + 3
    d1 = torch.from_numpy(rng.standard_normal((m, ld)).astype(np.float32)).to(DEV)
    nparts = -(-m // per)
    slab = int(lib.g2048_sized_onehot_dw1_slab(size, h1))
    assert slab == (17 * cells + 1) * h1
    part = _guarded(nparts * slab)
    L.check(lib.g2048_sized_onehot_dw1(size, L.ptr(planes), planes.shape[1], L.ptr(d1), h1, m, ld, per, L.ptr(part),
                                       nparts, st))
    torch.cuda.synchronize()
    assert _intact(part, nparts * slab) and torch.equal(planes, before)
    acc = torch.zeros(slab, dtype=torch.float64, device=DEV)
    L.check(lib.g2048_fold_partials(L.ptr(part), nparts, slab, L.ptr(acc), st))
    X, _ = _features(L, size, planes, m, "onehot", 1.0)
    dd = d1[:, :h1].double()
    ref_w, ref_b = X.t() @ dd, dd.sum(0)
    rows = 17 * cells
    got_w = acc[:rows * h1].view(rows, h1)
    # each slab element: an fp32 accumulation of the exact products of the one-hot with the three bf16 planes of every
    # delta (sum |d_i| <= (1 + 2^-7) |d|): bounded as a sequential fp32 sum of 3 per + 16 terms
    k = 3 * per + 16
    g = k * 2.0 ** -24 / (1 - k * 2.0 ** -24) * (1 + 2.0 ** -7)
    assert bool(((got_w - ref_w).abs() <= g * (X.t() @ dd.abs()) + 1e-30).all())
    g = per * 2.0 ** -24 / (1 - per * 2.0 ** -24)
    assert bool(((acc[rows * h1:] - ref_b).abs() <= g * dd.abs().sum(0) + 1e-30).all())
    seen = torch.zeros(rows, dtype=torch.bool, device=DEV)
    seen[(torch.arange(cells, device=DEV) * 17 + torch.from_numpy(e.astype(np.int64)).to(DEV)).reshape(-1)] = True
    assert bool((got_w[~seen] == 0).all())
    # deterministic: a second call gives the same bits
    part2 = _guarded(nparts * slab)
    L.check(lib.g2048_sized_onehot_dw1(size, L.ptr(planes), planes.shape[1], L.ptr(d1), h1, m, ld, per, L.ptr(part2),
                                       nparts, st))
    assert torch.equal(part, part2)


# ------------------------------------------------------------------------------------------------------- agent
def _agent(env, mlp, agent, fused=True):
    from rl2048_amd import Game2048EnvConfig
    from rl2048_amd.agent import ReinforceAgent, ReinforceAgentConfig
    from rl2048_amd.mlp import MLPConfig

    a = ReinforceAgent(Game2048EnvConfig(**env), MLPConfig(**mlp), ReinforceAgentConfig(**agent), device=DEV)
    a.use_fused_sized_grad = fused
    return a


AGENT_CASES = [
    ("N3-log2-reinforce", dict(size=3, obs_mode="log2", obs_log2_scale=0.25, reward_mode="log2", max_steps=40),
     dict(hidden_sizes=[32], activation="ReLU"), dict(gamma=0.99, baseline_mode="batch", model_seed=3), ""),
    ("N5-onehot-ac-aug", dict(size=5, obs_mode="onehot", reward_mode="sum", base_reward_scale=0.1, max_steps=40),
     dict(hidden_sizes=[64, 32], activation="ReLU"),
     dict(gamma=0.99, baseline_mode="batch", use_critic=True, augmentation=True, optimizer="adam", model_seed=5),
     " + g2048_sized_onehot_dw1"),
    ("N8-log2-ac-huber", dict(size=8, obs_mode="log2", obs_log2_scale=0.125, reward_mode="log2", max_steps=40),
     dict(hidden_sizes=[64, 64], activation="Sigmoid"),
     dict(gamma=0.99, baseline_mode="batch_norm", use_critic=True, critic_loss_type="huber", huber_delta=0.5,
          model_seed=8), ""),
]


def _norm(gs):
    return float(torch.sqrt(sum((g.double() ** 2).sum() for g in gs)))


@pytest.mark.parametrize("name,env,mlp,acfg,suffix", AGENT_CASES, ids=[c[0] for c in AGENT_CASES])
def test_agent_update_matches_fp64(name, env, mlp, acfg, suffix):
    agent = _agent(env, mlp, acfg)
    batch = agent.rollout_batch(list(range(64)), list(range(1000, 1064)))
    params = EG.snapshot(agent)
    stats = agent.update_from_batch(batch)
    paths = agent.last_paths()
    assert paths["actor_grad"] == "g2048_sized_grad" + suffix
    if acfg.get("use_critic"):
        assert paths["critic_grad"] == "g2048_sized_grad" + suffix
    flips = {}
    exact = _exact_update(agent, batch, params, flips)
    for v in flips.values():
        assert sum(v["viol"]) == 0, flips
    errs = EG.grad_errors(agent.last_grads, exact)
    print(f"\n{name}: {errs}")
    assert max(errs.values()) < BAR, errs
    assert abs(stats["actor_grad_norm"] - _norm(exact["actor"])) <= BAR * _norm(exact["actor"])
    if acfg.get("use_critic"):
        assert abs(stats["critic_grad_norm"] - _norm(exact["critic"])) <= BAR * _norm(exact["critic"])
    if mlp["activation"] == "Sigmoid":
        # the general path on the same batch and parameters: both within 1e-5 of the same fp64 value
        other = _agent(env, mlp, acfg, fused=False)
        other.params, other.critic_params = params
        other._params_version += 1
        other.update_from_batch(batch)
        assert other.last_paths()["actor_grad"] == "hipBLASLt backprop"
        assert other.last_paths()["critic_grad"] == "hipBLASLt backprop"
        assert max(EG.grad_errors(other.last_grads, exact).values()) < BAR
        both = EG.grad_errors(agent.last_grads, other.last_grads)
        assert max(both.values()) < 2 * BAR, both


def test_fall_throughs_keep_the_general_path():
    """An uncovered net and the drop-in update_batch (features, no boards) with the switch on: today's path strings."""
    env = dict(size=5, obs_mode="log2", obs_log2_scale=0.25, max_steps=12)
    big = _agent(env, dict(hidden_sizes=[256, 256, 256], activation="ReLU"), dict(use_critic=True, model_seed=1))
    assert big._sized_grad_spec(big.params, 4) is None
    batch = big.rollout_batch(list(range(8)), list(range(50, 58)))
    big.update_from_batch(batch)
    assert big.last_paths()["actor_grad"] == "hipBLASLt backprop"
    assert big.last_paths()["critic_grad"] == "hipBLASLt backprop"
    small = _agent(env, dict(hidden_sizes=[32], activation="ReLU"), dict(use_critic=True, model_seed=1))
    assert small._sized_grad_spec(small.params, 4) is not None
    b2 = small.rollout_batch(list(range(8)), list(range(50, 58)))
    small.update_batch(small.trajectories_from_batch(b2))
    assert small.last_paths()["actor_grad"] == "hipBLASLt backprop"
    assert small.last_paths()["critic_grad"] == "hipBLASLt backprop"
    small.update_from_batch(b2)
    assert small.last_paths()["actor_grad"] == "g2048_sized_grad"
    off = _agent(env, dict(hidden_sizes=[32], activation="ReLU"), dict(model_seed=1), fused=False)
    assert off._sized_grad_spec(off.params, 4) is None


# ------------------------------------------------------------------------------- the reference's recorded batches
D = RF.load("sized_agent")
FIX = json.loads(str(D["agent_cases"]))


def _params(ci, prefix, nl):
    flat = [D[f"a{ci}_{prefix}_{j}"] for j in range(2 * nl)]
    return {"W": [a.copy() for a in flat[:nl]], "b": [a.copy() for a in flat[nl:]]}


def _before(ci, u, nl, which):
    return _params(ci, f"init_{which}" if u == 0 else f"up{u - 1}_{which}", nl)


def _set(agent, params, critic=False):
    t = {k: [torch.from_numpy(a.copy()).to(DEV) for a in v] for k, v in params.items()}
    if critic:
        agent.critic_params = t
    else:
        agent.params = t
    agent._params_version += 1


def _batch(ci, u, case):
    """The reference's recorded batch as a TrajectoryBatch (restated from tests/test_gpu_sized_agent.py)."""
    from rl2048_amd.agent import TrajectoryBatch

    P, ns = f"a{ci}_up{u}_", case["env"]["size"]
    lens = D[P + "lengths"]
    n, T = len(lens), int(lens.max())
    ex = np.zeros((T, n, ns * ns), dtype=np.uint64)
    acts = np.zeros((T, n), dtype=np.uint8)
    rews = np.zeros((T, n), dtype=np.float64)
    s = 0
    for i, Ti in enumerate(lens):
        Ti = int(Ti)
        ex[:Ti, i] = D[P + "boards"][s:s + Ti]
        acts[:Ti, i] = D[P + "actions"][s:s + Ti]
        rews[:Ti, i] = D[P + "rewards"][s:s + Ti]
        s += Ti
    W = _words(ns)
    planes = np.zeros((W, T, n), dtype=np.uint64)
    for k in range(ns * ns):
        planes[k >> 4] |= ex[..., k] << np.uint64(4 * (k & 15))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    return TrajectoryBatch(boards=t(planes.view(np.int64)), actions=t(acts), rewards=t(rews),
                           flags=torch.zeros(T, n, dtype=torch.uint8, device=DEV), lengths=t(lens.astype(np.int32)),
                           total_reward=t(D[P + "total_reward"].copy()), max_tile=t(D[P + "max_tile"].copy()),
                           final_boards=torch.zeros(W, n, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize("ci", range(len(FIX)))
def test_reference_fixture_updates_through_the_fused_path(ci):
    """Both cases of tests/golden/sized_agent.npz through update_from_batch with the switch on: each gradient tensor
    within 1e-5 normwise of the reference's recorded one -- or, where a ReLU flip against the reference's fp32 run
    shows, within 1e-5 of fp64 under the kernel's own pattern with zero violations of the flip bound -- and the
    parameters after the step by the existing helpers."""
    case = FIX[ci]
    nl = len(case["mlp"]["hidden_sizes"]) + 1
    agent = _agent(case["env"], case["mlp"], case["agent"])
    crit = f"a{ci}_init_critic_0" in D
    lr = case["agent"].get("learning_rate", 1e-3)
    lr_c = case["agent"].get("critic_learning_rate", 1e-3)
    adam = case["agent"].get("optimizer", "sgd") == "adam"
    b1, b2 = case["agent"].get("adam_beta1", 0.9), case["agent"].get("adam_beta2", 0.999)
    mx = case["agent"].get("max_grad_norm", 1.0)
    onehot = case["env"]["obs_mode"] == "onehot"
    want = "g2048_sized_grad" + (" + g2048_sized_onehot_dw1" if onehot else "")
    noisy = {"actor": None, "critic": None}
    for u in range(case["updates"]):
        P = f"a{ci}_up{u}_"
        _set(agent, _before(ci, u, nl, "actor"))
        if crit:
            _set(agent, _before(ci, u, nl, "critic"), critic=True)
        snap = EG.snapshot(agent)
        batch = _batch(ci, u, case)
        ast = RF.adam_state(agent) if adam else None
        cst = RF.adam_state(agent, critic=True) if adam and crit else None
        agent.update_from_batch(batch)
        assert agent.last_paths()["actor_grad"] == want
        if crit:
            assert agent.last_paths()["critic_grad"] == want
        exact = {}

        def exact_of(which):
            if not exact:
                flips = {}
                exact.update(_exact_update(agent, batch, snap, flips))
                for v in flips.values():
                    assert sum(v["viol"]) == 0, flips
            return exact[which]

        for which, P_after, sign, lr_w, st in (("actor", agent.params, 1.0, lr, ast),
                                               ("critic", agent.critic_params, -1.0, lr_c, cst)):
            if which == "critic" and not crit:
                continue
            gref = [D[P + f"{which}_grad_{j}"] for j in range(2 * nl)]
            for j, (g, r) in enumerate(zip(agent.last_grads[which], gref)):
                if RF.rel(g.cpu().numpy(), r) >= BAR:
                    e = EG._rel(g, exact_of(which)[j])
                    assert e < BAR, (u, which, j, "vs reference", RF.rel(g.cpu().numpy(), r), "vs fp64", e)
            ref, rb = _params(ci, f"up{u}_{which}", nl), _before(ci, u, nl, which)
            before = [t.cpu().numpy() for t in snap[0 if which == "actor" else 1]["W"] +
                      snap[0 if which == "actor" else 1]["b"]]
            after = [p.cpu().numpy() for p in P_after["W"] + P_after["b"]]
            noisy[which] = assert_step_matches(after, before, ref["W"] + ref["b"], rb["W"] + rb["b"], gref,
                                               noisy[which], lr_w, adam)
            if adam:
                RF.assert_adam_step_exact(after, before, [g.cpu().numpy() for g in agent.last_grads[which]], st, lr_w,
                                          sign, b1, b2, mx, (u, which))
