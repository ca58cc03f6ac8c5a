"""Test helper: g2048_sized_grad / g2048_sized_onehot_dw1 called directly with guarded buffers (Run), and the fp64
value of update_batch's pre-clip gradients on a sized batch under the kernel's own ReLU pattern (_exact_update), built
from the pieces of tests/exact_grad.py.  Used by tests/test_gpu_sized_grad.py and tools/check_sized_grad_at_size.py."""
import ctypes

import numpy as np
import torch

import exact_grad as EG

DEV = torch.device("cuda", 0)
SENT = 12345.0
TAIL = 64
BAR = 1e-5


def _lib():
    from rl2048_amd import _lib as L

    L.ensure_device(DEV)
    return L


def _fwd64_bound(W, B, x, act):
    """fp64 forward and a rigorous bound on an fp32 evaluation's error (tests/test_gpu_deep.py): every layer's
    pre-activation is a sum of fan-in + 1 terms, one rounding per operation (+ 8 for the output layer's partial sums), so
    |z^ - z| <= gamma_n (|a^| |W| + |b|) + |W| |a^ - a| with n = fan-in + 10; ReLU passes the error through, Sigmoid
    scales it by 1/4 and adds its own rounding (4 ulp of a)."""
    u = 2.0 ** -24
    a, E = x, torch.zeros_like(x)
    for i, (w, b) in enumerate(zip(W, B)):
        wd, bd = w.double(), b.double()
        n = w.shape[0] + 10
        z = a @ wd + bd
        Ez = (n * u / (1 - n * u)) * ((a.abs() + E) @ wd.abs() + bd.abs()) + E @ wd.abs()
        if i == len(W) - 1:
            return z, Ez
        if act == "ReLU":
            a, E = torch.relu(z), Ez
        else:
            a = torch.sigmoid(z)
            E = 0.25 * Ez + 4 * u * a.abs()
    raise AssertionError("unreachable")


def _r32(h):
    return 32 * ((h + 31) // 32)


def _words(size):
    return (size * size + 15) // 16


def _planes(e: np.ndarray, size: int, stride: int) -> torch.Tensor:
    """uint8 exponents [n, N*N] -> int64 planes [W, stride]; lanes n.. hold all-ones sentinels."""
    n = e.shape[0]
    out = np.full((_words(size), stride), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    out[:, :n] = 0
    e = e.astype(np.uint64)
    for k in range(size * size):
        out[k >> 4, :n] |= e[:, k] << np.uint64(4 * (k & 15))
    return torch.from_numpy(out.view(np.int64)).to(DEV)


def _boards(rng, n, size, stride=None):
    e = rng.integers(0, 16, size=(n, size * size), dtype=np.uint8)
    return e, _planes(e, size, n if stride is None else stride)


def _net(rng, din, hidden, dout, w0_scale=1.0):
    dims = [din] + list(hidden) + [dout]
    W = [rng.standard_normal((dims[i], dims[i + 1])).astype(np.float32) / np.float32(np.sqrt(dims[i]))
         for i in range(len(dims) - 1)]
    W[0] = (W[0] * np.float32(w0_scale)).astype(np.float32)
    B = [(0.3 * rng.standard_normal(dims[i + 1])).astype(np.float32) for i in range(len(dims) - 1)]
    t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    return [t(w) for w in W], [t(b) for b in B]


def _mode(L, mode):
    return {"raw": L.OBS_RAW, "log2": L.OBS_LOG2, "onehot": L.OBS_ONEHOT}[mode]


def _pack(L, size, W, B, mode, hidden, dout):
    lib, st = L.lib(), L.stream_handle(DEV)
    harr = (ctypes.c_int32 * len(hidden))(*hidden)
    code = _mode(L, mode)
    sz = int(lib.g2048_sized_policy_packed_size(size, code, len(hidden), harr))
    packed = torch.empty(sz, dtype=torch.float32, device=DEV)
    wp = (ctypes.c_void_p * len(W))(*[w.data_ptr() for w in W])
    bp = (ctypes.c_void_p * len(B))(*[b.data_ptr() for b in B])
    L.check(lib.g2048_sized_pack(size, wp, bp, code, len(hidden), harr, dout, L.ptr(packed), sz, st))
    gsz = int(lib.g2048_deep_grad_pack_size(code, len(hidden), harr))
    gpacked = torch.empty(gsz, dtype=torch.float32, device=DEV)
    L.check(lib.g2048_deep_grad_pack(wp, code, len(hidden), harr, L.ptr(gpacked), gsz, st))
    return packed, gpacked, harr


def _features(L, size, planes, n, mode, scale):
    """(x [n, D] fp64, mask [n, 4] bool) by g2048_sized_obs."""
    D = size * size * (17 if mode == "onehot" else 1)
    x = torch.empty(n, D, dtype=torch.float32, device=DEV)
    mk = torch.empty(n, 4, dtype=torch.int8, device=DEV)
    L.check(L.lib().g2048_sized_obs(size, L.ptr(planes), planes.shape[1], _mode(L, mode), scale, L.ptr(x), L.ptr(mk), n,
                                    L.stream_handle(DEV)))
    return x.double(), mk.bool()


def _guarded(numel, dtype=torch.float32):
    t = torch.full((numel + TAIL,), SENT, dtype=dtype, device=DEV)
    return t


def _intact(t, numel):
    return bool((t[numel:] == SENT).all())


SCALE = 0.0625


class Run:
    """One g2048_sized_grad call (+ g2048_sized_onehot_dw1 on one-hot obs) with every buffer guarded, folded in fp64
    and unpacked into [dW_0..dW_L, db_0..db_L] by the agent's layout."""

    def __init__(self, L, size, mode, hidden, act, W, B, planes, n, critic, loss=0, huber_delta=1.0, actions=None,
                 coef=None, target=None, nparts=2, use_mask=1, want_hidden=True, packs=None, scale=SCALE):
        from rl2048_amd.agent import ReinforceAgent

        lib, st = L.lib(), L.stream_handle(DEV)
        dout = 1 if critic else 4
        nh, code = len(hidden), _mode(L, mode)
        packed, gpacked, harr = packs if packs is not None else _pack(L, size, W, B, mode, hidden, dout)
        pw, pb, rows0, slab = ReinforceAgent._sized_slab_layout(size, hidden, mode == "onehot")
        assert slab == lib.g2048_sized_grad_slab(size, code, nh, harr)
        Hp = [_r32(h) for h in hidden]
        before = planes.clone()
        part = _guarded(nparts * slab)
        delta, value = _guarded(n), _guarded(n)
        d0 = _guarded(n * Hp[0])
        hid = [_guarded(n * Hp[l]) for l in range(nh)]
        hp = (ctypes.c_void_p * nh)(*[h.data_ptr() for h in hid]) if want_hidden else None
        act_code = {"ReLU": L.ACT_RELU, "Sigmoid": L.ACT_SIGMOID}[act]
        L.check(lib.g2048_sized_grad(size, L.ptr(packed), L.ptr(gpacked), nh, harr, act_code, code, scale, use_mask,
                                     L.ptr(planes), planes.shape[1], L.ptr(actions), L.ptr(coef), int(critic), loss,
                                     huber_delta, L.ptr(target), L.ptr(delta) if critic else None,
                                     L.ptr(value) if critic else None, L.ptr(d0) if mode == "onehot" else None, hp, n,
                                     L.ptr(part), nparts, st))
        torch.cuda.synchronize()
        assert torch.equal(planes, before), "board planes (sentinel lanes included) were written"
        assert _intact(part, nparts * slab) and _intact(delta, n) and _intact(value, n) and _intact(d0, n * Hp[0])
        assert all(_intact(h, n * Hp[l]) for l, h in enumerate(hid))
        if not critic:
            assert bool((delta == SENT).all()) and bool((value == SENT).all())
        if mode != "onehot":
            assert bool((d0 == SENT).all())
        self.part = part[:nparts * slab].view(nparts, slab)
        self.delta, self.value = delta[:n], value[:n]
        self.d0 = d0[:n * Hp[0]].view(n, Hp[0])
        self.hidden = [h[:n * Hp[l]].view(n, Hp[l])[:, :hidden[l]] for l, h in enumerate(hid)] if want_hidden else None
        acc = torch.zeros(slab, dtype=torch.float64, device=DEV)
        L.check(lib.g2048_fold_partials(L.ptr(self.part), nparts, slab, L.ptr(acc), st))
        cells = size * size
        gW, gb = [], []
        if mode == "onehot":
            h0 = hidden[0]
            per = 64
            np1 = -(-n // per)
            s1 = int(lib.g2048_sized_onehot_dw1_slab(size, h0))
            p1 = _guarded(np1 * s1)
            L.check(lib.g2048_sized_onehot_dw1(size, L.ptr(planes), planes.shape[1], L.ptr(self.d0.contiguous()), h0, n,
                                               Hp[0], per, L.ptr(p1), np1, st))
            torch.cuda.synchronize()
            assert _intact(p1, np1 * s1) and torch.equal(planes, before)
            a1 = torch.zeros(s1, dtype=torch.float64, device=DEV)
            L.check(lib.g2048_fold_partials(L.ptr(p1), np1, s1, L.ptr(a1), st))
            gW.append(a1[:17 * cells * h0].view(17 * cells, h0))
        else:
            full = acc[pw[0]:pw[0] + rows0 * Hp[0]].view(rows0, Hp[0])
            assert bool((full[cells:] == 0).all()) and bool((full[:, hidden[0]:] == 0).all()), "dW_0 padding"
            gW.append(full[:cells, :hidden[0]])
        gb.append(acc[pb[0]:pb[0] + Hp[0]][:hidden[0]])
        for l in range(1, nh):
            gW.append(acc[pw[l]:pw[l] + Hp[l - 1] * Hp[l]].view(Hp[l - 1], Hp[l])[:hidden[l - 1], :hidden[l]])
            gb.append(acc[pb[l]:pb[l] + Hp[l]][:hidden[l]])
        gW.append(acc[pw[nh]:pw[nh] + Hp[-1] * 4].view(Hp[-1], 4)[:hidden[-1], :dout])
        gb.append(acc[pb[nh]:pb[nh] + 4][:dout])
        self.grads = gW + gb


def _loss_grad(critic, loss, hd, out, mk, actions, coef, target, use_mask=True):
    """update_batch's output-layer delta in fp64: the policy-gradient one (masked softmax) or the value loss's."""
    if not critic:
        lg = torch.where(mk, out, torch.full_like(out, -1e9)) if use_mask else out
        p = torch.softmax(lg, dim=1)
        oh = torch.nn.functional.one_hot(actions.long(), 4).double()
        return (oh - p) * coef.double().unsqueeze(1)
    diff = out[:, 0] - target.double()
    if loss == 1:
        diff = torch.where(diff.abs() <= hd, diff, hd * torch.sign(diff))
    return (diff * coef.double()).unsqueeze(1)


def _kernel_masks(agent, P, boards, out_dim):
    """The ReLU pattern of every hidden layer as g2048_sized_grad computes it on the planes `boards` [W, m]: the entry
    point itself with hidden_out (zero coefficients; the pattern is the forward's)."""
    L = _lib()
    sspec = agent._sized_spec(P, out_dim)
    obs_code, hidden, act, harr = sspec
    mode = {L.OBS_RAW: "raw", L.OBS_LOG2: "log2", L.OBS_ONEHOT: "onehot"}[obs_code]
    m = boards.shape[1]
    slot = "probe%d" % out_dim
    packs = (agent._pack_sized(P, sspec, slot, out_dim), agent._pack_deep_grad(P, sspec, slot), harr)
    r = Run(L, agent.size, mode, list(hidden), "ReLU", None, None, boards.contiguous(), m, False,
            actions=torch.zeros(m, dtype=torch.uint8, device=DEV), coef=torch.zeros(m, device=DEV), nparts=4,
            use_mask=int(bool(agent.env_config.use_action_mask)), packs=packs,
            scale=float(agent.env_config.obs_log2_scale))
    return [h > 0 for h in r.hidden]


def _exact_update(agent, batch, params, flip_stats=None):
    """update_batch's pre-clip gradients {"actor", "critic"} in fp64 on a sized batch (any K, baseline off / batch /
    batch_norm, MSE / Huber, no rank weights), ReLU nets under the kernel's own pattern (_kernel_masks)."""
    from rl2048_amd.agent import _Steps

    actor_p, critic_p = params
    c, act = agent.agent_config, agent.mlp_config.activation
    assert not c.reward_rank_weights
    K = 8 if c.augmentation else 1
    steps = _Steps(agent, batch.lengths, batch.actions, batch.rewards, boards=batch.boards)
    n, N = steps.n, steps.N
    sel = torch.arange(N, device=DEV)
    w_step = 1.0 / (steps.lengths[steps.lane].double() * (K * n))
    use_mask = bool(agent.env_config.use_action_mask)
    net64 = lambda P: ([w.double() for w in P["W"]], [v.double() for v in P["b"]])   # noqa: E731

    def fwd(P, W, b, k, key, out_dim):
        bk = steps.boards_at(sel, k)
        x, mk = agent._obs_from_boards(bk)
        x = x.double()
        m = _kernel_masks(agent, P, bk, out_dim) if act == "ReLU" else None
        if flip_stats is not None and m is not None:
            EG.pattern_flip_check_deep(W, b, x, EG.fwd64_deep(W, b, x, act)[0], m, flip_stats, key)
        return EG.fwd64_deep(W, b, x, act, m), mk

    out = {}
    if c.use_critic:
        Wc, bc = net64(critic_p)
        accc = [torch.zeros_like(p) for p in Wc + bc]
        delta = torch.empty(K, N, dtype=torch.float64, device=DEV)
        for k in range(K):
            (zs, acts, v), _ = fwd(critic_p, Wc, bc, k, "critic", 1)
            xn = agent._obs_from_boards(steps.boards_at(sel, k, nxt=True))[0].double()
            vn = EG.fwd64_deep(Wc, bc, xn, act)[2][:, 0]
            tgt = steps.rewards.double() + c.gamma * vn * steps.has_next.double()
            delta[k] = tgt - v[:, 0]
            diff = v[:, 0] - tgt
            if c.critic_loss_type == "huber":
                diff = torch.where(diff.abs() <= c.huber_delta, diff, c.huber_delta * torch.sign(diff))
            EG.bwd64_deep(Wc, zs, acts, (diff * w_step).unsqueeze(1), accc, act)
        out["critic"] = accc
        values = delta.float().double()
    else:
        T = steps.T
        G = torch.zeros(n, dtype=torch.float64, device=DEV)
        Gt = torch.empty(T, n, dtype=torch.float64, device=DEV)
        R64 = batch.rewards.double()
        for tt in reversed(range(T)):
            G = R64[tt] + c.gamma * G
            Gt[tt] = G
        values = Gt.float().double().reshape(-1)[steps.vidx].unsqueeze(0).expand(K, -1)
    mode = c.baseline_mode
    if mode in ("batch", "batch_norm"):
        mu = values.mean()
        adv = values - mu
        if mode == "batch_norm":
            adv = adv / ((values - mu).pow(2).mean().sqrt()).clamp_min(1e-8)
    else:
        assert mode == "off", mode
        adv = values
    W, b = net64(actor_p)
    acc = [torch.zeros_like(p) for p in W + b]
    for k in range(K):
        (zs, acts, lg), mk = fwd(actor_p, W, b, k, "actor", 4)
        if use_mask:
            lg = torch.where(mk.bool(), lg, torch.full_like(lg, -1e9))
        p = torch.softmax(lg, dim=1)
        oh = torch.nn.functional.one_hot(EG.actions_k(steps.actions, k), 4).double()
        EG.bwd64_deep(W, zs, acts, (oh - p) * (adv[k] * w_step).unsqueeze(1), acc, act)
    out["actor"] = acc
    return out
