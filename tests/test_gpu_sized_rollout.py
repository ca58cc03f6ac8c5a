"""GPU: g2048_sized_rollout (csrc/g2048_sized_rollout.hip), the persistent whole-rollout kernel for board sizes 2..8,
and the agent's rollout through it (ReinforceAgent.use_fused_sized_rollout).

The yardstick throughout is the per-step fused path -- the same agent with use_fused_sized_rollout off and
use_fused_sized_policy on, on the same seeds.  Both run the same forward (sized_forward), choice (softmax_select) and
env step (sized::env_step), so the comparison is bit for bit: torch.equal, no tolerance.  On valid rows
(t < lengths[e]): every board plane, actions, fp64 rewards, flags & ~F_INACTIVE, probabilities; per episode: lengths,
totals, max tile, final boards.  The suspend / resume test also replays episodes in tests/sized_ref.py's NumPy env with
numpy's Generator.choice on the recorded probabilities, the reference test compares with the real reference's
recorded episodes (tests/golden/sized_agent.npz), and size 4 through the new entry point is compared with
g2048_deep_rollout.
"""
import ctypes
import json

import numpy as np
import pytest
import torch

import sized_ref as SR
from test_gpu_deep import _net

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

NEW_PATH = "g2048_sized_rollout (persistent launches, suspended episodes resumed)"
STEP_PATH = "g2048_sized_policy + g2048_sized_step per step (active lanes)"
GENERAL = "hipBLASLt forward (active lanes) + g2048_sample + g2048_sized_step per step"
BASE_ENV = dict(obs_log2_scale=0.125, max_steps=40, use_action_mask=True, reward_mode="log2", empty_tile_reward=0.05)
NET_LOG2 = ("log2", [48], "ReLU")
NET_ONEHOT = ("onehot", [32, 16], "Sigmoid")


def _agent(size, net, env=None, seed=None):
    from rl2048_amd import Game2048EnvConfig
    from rl2048_amd.agent import ReinforceAgent, ReinforceAgentConfig
    from rl2048_amd.mlp import MLPConfig

    mode, hidden, act = net
    cfg = Game2048EnvConfig(size=size, obs_mode=mode, **dict(BASE_ENV, **(env or {})))
    a = ReinforceAgent(cfg, MLPConfig(hidden_sizes=hidden, activation=act, init_distribution="HeNormal"),
                       ReinforceAgentConfig(model_seed=size if seed is None else seed), device=DEV)
    if size == 4:
        # The agent never routes 4 x 4 boards to the sized entry points (they accept N = 4, W = 1).  This one is
        # re-pointed at them: the 4 x 4 kernels off, its env through tests/sized_ref.as_sized4.
        a._sized, a.use_fused_policy, a.use_fused_rollout = True, False, False
        assert a._fused_policy_spec() is None
        make = a._vec_env

        def vec(n, rng):
            env = make(n, rng)
            return env if env._sized else SR.as_sized4(env)

        a._vec_env = vec
    return a


def _both(agent, es, ps, greedy=False):
    """(persistent batch, per-step fused batch) of the same agent on the same seeds."""
    agent.use_fused_sized_rollout, agent.use_fused_sized_policy = True, False
    b1 = agent.rollout_batch(es, ps, use_greedy=greedy, record_probs=True)
    assert agent.last_paths()["rollout"] == NEW_PATH
    agent.use_fused_sized_rollout, agent.use_fused_sized_policy = False, True
    b2 = agent.rollout_batch(es, ps, use_greedy=greedy, record_probs=True)
    assert agent.last_paths()["rollout"] == STEP_PATH
    return b1, b2


def _assert_equal(b1, b2, size):
    from rl2048_amd import _lib as L

    W, n = SR.words(size), b2.n
    assert torch.equal(b1.lengths, b2.lengths) and b1.T == b2.T == int(b2.lengths.max())
    for name in ("boards", "actions", "rewards", "flags", "probs", "lengths", "total_reward", "max_tile", "final_boards"):
        x, y = getattr(b1, name), getattr(b2, name)
        assert x.dtype == y.dtype and tuple(x.shape) == tuple(y.shape), name
    assert tuple(b1.boards.shape) == (W, b1.T, n) and tuple(b1.final_boards.shape) == (W, n)
    valid = torch.arange(b1.T, device=DEV).unsqueeze(1) < b1.lengths.unsqueeze(0)
    assert int(valid.sum()) == int(b1.lengths.sum())
    for w in range(W):
        assert torch.equal(b1.boards[w][valid], b2.boards[w][valid]), f"boards plane {w}"
    for name in ("actions", "rewards", "probs"):
        assert torch.equal(getattr(b1, name)[valid], getattr(b2, name)[valid]), name
    assert torch.equal((b1.flags & ~L.F_INACTIVE)[valid], (b2.flags & ~L.F_INACTIVE)[valid])
    assert bool(((b1.flags & L.F_INACTIVE) != 0)[~valid].all())         # rows past an episode's end stay inactive
    assert torch.equal(b1.total_reward, b2.total_reward) and torch.equal(b1.max_tile, b2.max_tile)
    assert torch.equal(b1.final_boards, b2.final_boards)


def _endings(b):
    """(episodes that terminated, episodes that were truncated) from the last valid row's flags."""
    from rl2048_amd import _lib as L

    last = b.flags.gather(0, (b.lengths.long() - 1).unsqueeze(0))[0]
    return int(((last & L.F_TERMINATED) != 0).sum()), int(((last & L.F_TRUNCATED) != 0).sum())


def _seeds(n, base):
    es = np.arange(base, base + n, dtype=np.int64)
    return es, es + 10 ** 9


# ------------------------------------------------------------------------- 1. every size, both first-layer forms
SIZE_CASES = [(s, net, None, False) for s in range(2, 9) for net in (NET_LOG2, NET_ONEHOT)] + [
    (6, NET_LOG2, dict(reward_mode="sum", base_reward_scale=0.3, empty_tile_reward=0.0), False),   # non-dyadic scale
    (3, NET_ONEHOT, None, True),                                                                   # greedy
    (7, NET_LOG2, dict(use_action_mask=False, invalid_action_penalty=-0.7), False),
]
_done_cases: dict = {}


def _run_size_case(ci):
    if ci not in _done_cases:
        size, net, env, greedy = SIZE_CASES[ci]
        a = _agent(size, net, env)
        assert a._sized_spec() is not None
        es, ps = _seeds(97, 31_000 + 1000 * ci)                # three full groups plus a ragged one
        b1, b2 = _both(a, es, ps, greedy)
        _assert_equal(b1, b2, size)
        term, trunc = _endings(b1)
        assert term + trunc == 97 and int(b1.lengths.min()) >= 1 and int(b1.lengths.max()) <= 40
        _done_cases[ci] = (term, trunc)
    return _done_cases[ci]


@pytest.mark.parametrize("ci", range(len(SIZE_CASES)),
                         ids=[f"N{s}-{n[0]}{'-' + '-'.join(e) if e else ''}{'-greedy' if g else ''}"
                              for s, n, e, g in SIZE_CASES])
def test_every_size_equals_the_per_step_path(ci):
    """N in 2..8 (W = 1, 1, 1, 2, 3, 4, 4) x (log2 [48] ReLU, one-hot [32, 16] Sigmoid), n = 97, max_steps = 40, mask
    on, log2 reward with empty_tile_reward; plus the sum reward with a non-dyadic scale, greedy, and no mask with an
    invalid-action penalty."""
    _run_size_case(ci)


def test_both_endings_occur():
    """Small boards end by termination, large ones by truncation: each at least once across the cases above."""
    ends = [_run_size_case(ci) for ci in range(len(SIZE_CASES))]
    assert sum(t for t, _ in ends) > 0 and sum(u for _, u in ends) > 0
    assert ends[0][0] > 0          # N = 2 terminates
    assert ends[12][1] > 0         # N = 8 is truncated at 40 steps


# ------------------------------------------------------------------------------------------------ 2. ragged counts
@pytest.mark.parametrize("n", [1, 31, 32, 33])
def test_ragged_episode_counts(n):
    a = _agent(5, NET_ONEHOT)
    es, ps = _seeds(n, 52_000)
    b1, b2 = _both(a, es, ps)
    _assert_equal(b1, b2, 5)


# -------------------------------------------------------------------------------------------------- 3. slot refill
@pytest.mark.parametrize("size", [3, 6, 8])
def test_slots_refill_from_the_queue(size):
    """Two workgroups = 64 slots for 300 episodes: every slot plays about five episodes and the last claims run past
    n_order."""
    a = _agent(size, NET_LOG2 if size != 6 else NET_ONEHOT)
    a.sized_rollout_max_workgroups = 2
    es, ps = _seeds(300, 63_000)
    b1, b2 = _both(a, es, ps)
    _assert_equal(b1, b2, size)
    a.use_fused_sized_rollout = True
    a.rollout_batch(es[:5], ps[:5])
    assert a.last_paths()["rollout"] == NEW_PATH


# --------------------------------------------------------------------------------------------- 4. suspend / resume
@pytest.mark.parametrize("size,max_steps", [(3, None), (5, 70)])
def test_suspend_resume_equals_stepwise_and_the_numpy_env(size, max_steps):
    """First capacity 8 rows: every episode is suspended and resumed as the buffer doubles (N = 3, max_steps None:
    until termination; N = 5: the cap is below max_steps = 70, so truncation comes from the restored step count).
    Equal to the per-step path, and a handful of episodes replayed in the NumPy env of tests/sized_ref.py with
    numpy's Generator.choice on the recorded probabilities."""
    env = dict(max_steps=max_steps)
    a = _agent(size, NET_ONEHOT, env)
    a.sized_rollout_cap0 = 8
    n = 257
    es, ps = _seeds(n, 74_000)
    b1, b2 = _both(a, es, ps)
    assert b1.T > 8
    _assert_equal(b1, b2, size)
    term, trunc = _endings(b1)
    assert (trunc == 0 and term == n) if max_steps is None else trunc > 0
    cfg = dict(BASE_ENV, obs_mode="onehot", max_steps=max_steps)
    lens = b1.lengths.cpu().numpy()
    boards = SR.unpack_planes(b1.boards.cpu().numpy(), size)             # [T, n, N*N]
    acts, rews, probs = b1.actions.cpu().numpy(), b1.rewards.cpu().numpy(), b1.probs.cpu().numpy()
    picks = [0, 1, n // 2, n - 1, int(lens.argmax())] + list(np.random.default_rng(0).choice(n, 6, replace=False))
    for i in picks:
        e = SR.SizedRef(size, cfg)
        e.reset(int(es[i]))
        pol = np.random.default_rng(int(ps[i]))
        total = 0.0
        for t in range(int(lens[i])):
            np.testing.assert_array_equal(boards[t, i], SR.exponents(e.board).reshape(-1), err_msg=f"{i}, {t}")
            assert int(pol.choice(4, p=probs[t, i])) == int(acts[t, i]), (i, t)
            r = e.step(int(acts[t, i]))
            assert rews[t, i] == r["reward"], (i, t)
            total += r["reward"]
            assert (r["terminated"] or r["truncated"]) == (t == lens[i] - 1), (i, t)
        assert float(b1.total_reward[i]) == total
        assert int(b1.max_tile[i]) == e.max_tile_seen


# ------------------------------------------------------------------------------------------------------ 5. refusal
def test_refuses_unbounded_growth():
    a = _agent(5, NET_LOG2, dict(max_steps=None))
    a.use_fused_sized_rollout = True
    a.sized_rollout_cap0, a.sized_rollout_max_rows = 8, 12
    es, ps = _seeds(64, 85_000)
    with pytest.raises(RuntimeError, match="still running after 8 steps"):
        a.rollout_batch(es, ps)
    a.sized_rollout_max_rows = 1 << 24                     # and the same agent then rolls out normally
    b = a.rollout_batch(es, ps)
    assert a.last_paths()["rollout"] == NEW_PATH
    assert b.T > 8 and int(b.lengths.min()) > 0


# -------------------------------------------------------------- 6. size 4 through the new entry point == deep rollout
@pytest.mark.parametrize("mode,hidden", [("log2", [64, 48, 32]), ("onehot", [128, 64])])
def test_size4_equals_deep_rollout(mode, hidden):
    """Direct ctypes calls (the agent never routes size 4 here).  The one-hot case compares the 32-slot sized forward
    with the 64-slot deep_forward64; include/g2048.h promises the same bits from every one-hot forward."""
    from rl2048_amd import Game2048EnvConfig
    from rl2048_amd import _lib as L
    from rl2048_amd.config import env_cfg_struct

    L.ensure_device(DEV)
    lib, st = L.lib(), L.stream_handle(DEV)
    code = {"log2": L.OBS_LOG2, "onehot": L.OBS_ONEHOT}[mode]
    rng = np.random.default_rng(96 + len(hidden))
    W, B = _net(rng, 16 * (17 if mode == "onehot" else 1), hidden, 4)
    harr = (ctypes.c_int32 * len(hidden))(*hidden)
    wp = (ctypes.c_void_p * len(W))(*[w.data_ptr() for w in W])
    bp = (ctypes.c_void_p * len(B))(*[b.data_ptr() for b in B])
    ssize = int(lib.g2048_sized_policy_packed_size(4, code, len(hidden), harr))
    dsize = int(lib.g2048_deep_packed_size(code, len(hidden), harr))
    spacked = torch.empty(ssize, dtype=torch.float32, device=DEV)
    dpacked = torch.empty(dsize, dtype=torch.float32, device=DEV)
    L.check(lib.g2048_sized_pack(4, wp, bp, code, len(hidden), harr, 4, L.ptr(spacked), ssize, st))
    L.check(lib.g2048_deep_pack(wp, bp, code, len(hidden), harr, 4, L.ptr(dpacked), dsize, st))
    n, cap = 200, 60
    cfg = env_cfg_struct(Game2048EnvConfig(size=4, obs_mode=mode, **dict(BASE_ENV, max_steps=cap)))
    es, ps = _seeds(n, 97_000)
    outs = []
    for sized in (True, False):
        streams = []
        for seeds in (es, ps):
            sd = torch.from_numpy(seeds).to(DEV)
            rs = torch.empty(2 * n, dtype=torch.int64, device=DEV)
            inc = torch.empty(2 * n, dtype=torch.int64, device=DEV)
            buf = torch.empty(n, dtype=torch.int64, device=DEV)
            L.check(lib.g2048_seed_pcg64(L.ptr(sd), L.ptr(rs), L.ptr(inc), L.ptr(buf), n, st))
            streams += [rs, inc, buf]
        boards = torch.zeros(cap, n, dtype=torch.int64, device=DEV)
        actions = torch.zeros(cap, n, dtype=torch.uint8, device=DEV)
        rewards = torch.zeros(cap, n, dtype=torch.float64, device=DEV)
        flags = torch.full((cap, n), L.F_INACTIVE, dtype=torch.uint8, device=DEV)
        probs = torch.zeros(cap, n, 4, dtype=torch.float32, device=DEV)
        lengths = torch.zeros(n, dtype=torch.int32, device=DEV)
        totals = torch.zeros(n, dtype=torch.float64, device=DEV)
        max_e = torch.zeros(n, dtype=torch.uint8, device=DEV)
        final = torch.zeros(n, dtype=torch.int64, device=DEV)
        sus_t = [torch.zeros(n, dtype=torch.int64, device=DEV), torch.zeros(3 * n, dtype=torch.int32, device=DEV),
                 torch.zeros(n, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV),
                 torch.zeros(1, dtype=torch.int32, device=DEV)]
        sus = L.Suspend(*[L.ptr(t) for t in sus_t])
        traj = L.Traj(*[L.ptr(t) for t in (boards, actions, rewards, flags, probs, lengths, totals, max_e, final)])
        queue = torch.zeros(1, dtype=torch.int32, device=DEV)
        head = (len(hidden), harr, L.ACT_RELU, ctypes.byref(cfg), 0, *[L.ptr(t) for t in streams], L.ptr(queue), None,
                n, 0, ctypes.byref(sus), n, cap, ctypes.byref(traj))
        if sized:
            L.check(lib.g2048_sized_rollout(4, L.ptr(spacked), *head, cap * n, 0, st))
        else:
            L.check(lib.g2048_deep_rollout(L.ptr(dpacked), *head, st))
        torch.cuda.synchronize()
        assert int(sus_t[4].item()) == 0
        outs.append((boards, actions, rewards, flags, probs, lengths, totals, max_e, final, streams[0], streams[3]))
    s, d = outs
    assert torch.equal(s[5], d[5]) and int(s[5].min()) >= 1 and int(s[5].max()) <= cap
    valid = torch.arange(cap, device=DEV).unsqueeze(1) < s[5].unsqueeze(0)
    for k, name in enumerate(("boards", "actions", "rewards", "flags", "probs")):
        assert torch.equal(s[k][valid], d[k][valid]), name
    for k, name in ((6, "totals"), (7, "max_tile"), (8, "final_board")):
        assert torch.equal(s[k], d[k]), name
    assert len(torch.unique(s[1][valid])) == 4


# ------------------------------------------------------------------------------------------ 7. the reference itself
@pytest.mark.parametrize("ci", [0, 1])
def test_agent_rollout_matches_reference(ci):
    """tests/test_gpu_sized_policy.py::test_agent_rollout_matches_reference with the persistent rollout switched on:
    the real reference's recorded episodes (size 3 log2 [32], size 5 one-hot [64, 32]); exact lengths, actions,
    boards, fp64 rewards, totals and max tile, probabilities within the fixture's 2e-6."""
    import test_gpu_sized_agent as SA

    D, case = SA.D, SA.CASES[ci]
    n_size, nl = case["env"]["size"], len(case["mlp"]["hidden_sizes"]) + 1
    assert (n_size, case["env"]["obs_mode"], case["mlp"]["hidden_sizes"]) in ((3, "log2", [32]), (5, "onehot", [64, 32]))
    agent = SA._agent(case)
    assert agent.use_fused_sized_rollout is False
    agent.use_fused_sized_rollout = True
    assert agent._sized_spec() is not None
    for u in range(case["updates"]):
        P = f"a{ci}_up{u}_"
        assert (D[P + "margin"] >= 1e-4).all()
        SA._set(agent, SA._before(ci, u, nl, "actor"))
        es, ps = [int(s) for s in D[P + "env_seeds"]], [int(s) for s in D[P + "policy_seeds"]]
        batch = agent.rollout_batch(es, ps, record_probs=True)
        assert agent.last_paths()["rollout"] == NEW_PATH
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


# ------------------------------------------------------------------------------------------------------ 8. runner
def test_runner_matches_reference_training(tmp_path, monkeypatch):
    """tests/test_gpu_sized_agent.py::test_runner_matches_reference_training with the switch turned on for the agent
    the runner constructs: every CSV row exactly, the final actor within that test's tolerances."""
    import test_gpu_sized_agent as SA
    from rl2048_amd import runner as R
    from rl2048_amd.agent import ReinforceAgent

    D = SA.D
    conf = json.loads(str(D["r_conf"]))
    assert (D["r_margin"] >= 1e-4).all()
    monkeypatch.setattr(ReinforceAgent, "use_fused_sized_rollout", True)
    R.reset_defaults()
    try:
        R.apply_config_overrides_from_dict(conf)
        agent, ec, mc, ac, tc = R.build_training_components(DEV)
        assert ec.size == 3 and agent.size == 3 and agent.use_fused_sized_rollout is True
        rows = R.training_loop(agent, ec, mc, ac, tc, tmp_path, "golden")
        assert agent.last_paths()["rollout"] == NEW_PATH
        assert [r["batch"] for r in rows] == list(D["r_batch"])
        for k in ("avg_reward", "max_reward", "min_reward"):
            np.testing.assert_array_equal([r[k] for r in rows], D["r_" + k], err_msg=k)
        assert [json.loads(r["max_tile_counts"]) for r in rows] == D["r_max_tile_counts"].tolist()
        header = (tmp_path / "training_stats.csv").read_text().splitlines()[0].split(",")
        assert header == json.loads(str(D["r_csv_header"]))
        lr = conf["agent"]["learning_rate"]
        for j, p in enumerate(agent.params["W"] + agent.params["b"]):
            np.testing.assert_allclose(p.cpu().numpy(), D[f"r_final_actor_{j}"], rtol=1e-6, atol=2 * lr * 1e-5 + 1e-7,
                                       err_msg=f"tensor {j}")
    finally:
        R.reset_defaults()


# ------------------------------------------------------------------------------------------------ 9. fall-throughs
def test_fall_throughs_keep_todays_paths():
    es, ps = list(range(16)), list(range(16, 32))
    a = _agent(6, NET_LOG2, dict(max_steps=24))
    a.use_fused_sized_rollout, a.use_fused_sized_policy = True, True
    a.rollout_batch(es, ps, rng="philox")                  # Philox: the per-step fused policy
    assert a.last_paths()["rollout"] == STEP_PATH
    a.use_fused_sized_policy = False
    a.rollout_batch(es, ps, rng="philox")
    assert a.last_paths()["rollout"] == GENERAL
    a.rollout_batch(es, ps)                                # PCG64: the persistent rollout
    assert a.last_paths()["rollout"] == NEW_PATH
    a.use_fused_sized_rollout = False                      # the switch off: exactly today's strings
    a.rollout_batch(es, ps)
    assert a.last_paths()["rollout"] == GENERAL
    a.use_fused_sized_policy = True
    a.rollout_batch(es, ps)
    assert a.last_paths()["rollout"] == STEP_PATH
    u = _agent(6, ("log2", [300, 16], "ReLU"), dict(max_steps=24))   # a net the kernels do not cover
    u.use_fused_sized_rollout = True
    assert u._sized_spec() is None
    b = u.rollout_batch(es, ps)
    assert u.last_paths()["rollout"] == GENERAL
    ln = b.lengths.cpu().numpy()
    assert (ln >= 1).all() and (ln <= 24).all() and bool(torch.isfinite(b.total_reward).all())
