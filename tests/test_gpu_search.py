"""GPU: the expectimax player (rollout_batch / evaluate_batch / run_episode / evaluation_loop with action_gen =
ExpectimaxPolicy, agent.search_actions; g2048_*search_* of include/g2048_search.h).

* the fixture episodes (tests/golden/search.npz: the real reference's run_episode with the player as action_gen) row
  for row, evaluate_batch == rollout_batch, last_paths() names the new kernels;
* search_actions and the direct *_search_choose calls on the fixture boards of every size and depth (294 boards: more
  than one workgroup, no multiple of 64), sentinels around the outputs, q = NULL;
* refilled lanes and repeated suspensions (one workgroup, 256 + 229 episodes, first capacity = step budget = 16):
  every row replays in the CPU oracles (tests/rollout_replay.py) and every row's action equals the host build of the
  player (tests/native/search_host.cpp) on that row's board, mask on and off; one depth-2 case;
* direct C calls on a strict subset of the episodes (sentinels, policy streams byte-identical);
* run_episode's device path == its host path driven by the Python callable; update_from_batch on a search teacher
  batch == update_batch on the same trajectories; the runner's evaluation_loop.

Every comparison is ==.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import rollout_replay as RR
import sized_ref as SR
from test_search_host import BOARD_SIZES, ep_cases, fixture_boards, golden, native_choose

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROLL = {False: "g2048_search_rollout (persistent launches, one episode and one expectimax per lane, suspended episodes "
               "resumed)",
        True: "g2048_sized_search_rollout (persistent launches, one episode and one expectimax per lane, suspended "
              "episodes resumed)"}
EVAL = {False: "g2048_search_eval (persistent launches, one episode and one expectimax per lane, no trajectory rows, "
               "suspended episodes resumed)",
        True: "g2048_sized_search_eval (persistent launches, one episode and one expectimax per lane, no trajectory "
              "rows, suspended episodes resumed)"}
_done: dict = {}            # case id -> (agent, env seeds, policy seeds, policy, batch, counts): computed once


@pytest.fixture(scope="module")
def gold():
    return golden()


def _agent(env: dict, size=4, cap0=16, budget=16, max_workgroups=1, **agent_kw):
    from rl2048_amd import Game2048EnvConfig
    from rl2048_amd.agent import ReinforceAgent, ReinforceAgentConfig
    from rl2048_amd.mlp import MLPConfig

    a = ReinforceAgent(Game2048EnvConfig(size=size, **env), MLPConfig(hidden_sizes=[8], activation="ReLU"),
                       ReinforceAgentConfig(model_seed=3, **agent_kw), device=DEV)
    a.search_rollout_cap0, a.search_step_budget, a.search_max_workgroups = cap0, budget, max_workgroups
    return a


def _policy(depth, **kw):
    from rl2048_amd import ExpectimaxPolicy

    return ExpectimaxPolicy(depth=depth, **kw)


def _same_eval(ev, b):
    assert ev.lengths.dtype == b.lengths.dtype and torch.equal(ev.lengths, b.lengths)
    assert ev.total_reward.dtype == torch.float64
    assert torch.equal(ev.total_reward.view(torch.int64), b.total_reward.view(torch.int64))     # fp64 totals by bits
    assert ev.max_tile.dtype == b.max_tile.dtype and torch.equal(ev.max_tile, b.max_tile)
    assert ev.final_boards.shape == b.final_boards.shape and torch.equal(ev.final_boards, b.final_boards)


# ------------------------------------------------------------------------------------------ the reference's episodes
@pytest.mark.parametrize("c", range(8))
def test_fixture_episodes(gold, c):
    case = ep_cases()[c]
    size, depth = case["size"], case["depth"]
    a = _agent(case["env"], size=size, cap0=16, max_workgroups=0)
    P = f"e{c}_"
    lens = gold[P + "length"]
    start = np.concatenate([[0], np.cumsum(lens)])
    es, ps = gold[P + "env_seed"].astype(np.int64), gold[P + "policy_seed"].astype(np.int64)
    b = a.rollout_batch(es, ps, action_gen=_policy(depth))
    assert a.last_paths()["rollout"] == ROLL[size != 4] and b.probs is None
    np.testing.assert_array_equal(b.lengths.cpu().numpy(), lens)
    planes = b.boards.cpu().numpy() if size != 4 else b.boards.cpu().numpy()[None]
    ex = SR.unpack_planes(planes, size)
    acts, rews = b.actions.cpu().numpy(), b.rewards.cpu().numpy()
    for i in range(len(lens)):
        T, s = int(lens[i]), int(start[i])
        where = f"{case['name']} episode {i}"
        np.testing.assert_array_equal(ex[:T, i], gold[P + "boards"][s:s + T], err_msg=where)
        np.testing.assert_array_equal(acts[:T, i], gold[P + "actions"][s:s + T], err_msg=where)
        np.testing.assert_array_equal(rews[:T, i].view(np.uint64), gold[P + "rewards"][s:s + T].view(np.uint64),
                                      err_msg=where)
    np.testing.assert_array_equal(b.total_reward.cpu().numpy().view(np.uint64), gold[P + "total_reward"].view(np.uint64))
    np.testing.assert_array_equal(b.max_tile.cpu().numpy(), gold[P + "max_tile"])
    _same_eval(a.evaluate_batch(es, ps, action_gen=_policy(depth)), b)
    assert a.last_paths()["eval"] == EVAL[size != 4]


# ------------------------------------------------------------------------------------------------- single choices
CHOOSE_CASES = [(n, d) for n in BOARD_SIZES for d in (0, 1)] + [(n, 2) for n in (2, 3, 4)]


@pytest.mark.parametrize("size,depth", CHOOSE_CASES, ids=[f"N{n}-d{d}" for n, d in CHOOSE_CASES])
def test_search_actions_and_direct_choose_on_the_fixture_boards(gold, size, depth):
    from rl2048_amd import _lib as L

    e, q, act = fixture_boards(gold, size, depth)
    m = len(e)
    assert m % 64 != 0 and (depth == 2 or m > L.SCRIPT_BLOCK)
    planes = torch.from_numpy(SR.pack_planes(e, size)).to(DEV)                   # [W, m]
    a = _agent(dict(max_steps=None), size=size)
    pol = _policy(depth)
    got_a, got_q = a.search_actions(planes if size != 4 else planes[0], pol)
    assert got_a.dtype == torch.uint8 and got_q.dtype == torch.int64 and got_a.shape == (m,) and got_q.shape == (m, 4)
    np.testing.assert_array_equal(got_q.cpu().numpy(), q)
    np.testing.assert_array_equal(got_a.cpu().numpy(), act)
    assert "search_choose" in a.last_paths()["search_actions"]
    # any leading shape: TrajectoryBatch.boards as it is
    k = m // 2
    shaped = planes[:, :2 * k].reshape(-1, 2, k) if size != 4 else planes[0, :2 * k].reshape(2, k)
    sa, sq = a.search_actions(shaped, pol)
    assert sa.shape == (2, k) and sq.shape == (2, k, 4)
    np.testing.assert_array_equal(sa.cpu().numpy().reshape(-1), act[:2 * k])
    np.testing.assert_array_equal(sq.cpu().numpy().reshape(-1, 4), q[:2 * k])
    # the direct calls: sentinels past the outputs' used part, q = NULL
    pad, S8, S64 = 5, 0xA5, -0x5A5A5A5A5A5A5A5B
    sp = pol._search()
    for with_q in (True, False):
        actions = torch.full((m + pad,), S8, dtype=torch.uint8, device=DEV)
        qbuf = torch.full((m + pad, 4), S64, dtype=torch.int64, device=DEV)
        args = (ctypes.byref(sp), L.ptr(planes), m, L.ptr(actions), L.ptr(qbuf) if with_q else None, a._stream)
        if size != 4:
            L.check(a._lib.g2048_sized_search_choose(size, *args))
        else:
            L.check(a._lib.g2048_search_choose(*args))
            acts4 = torch.full((m + pad,), S8, dtype=torch.uint8, device=DEV)     # ... and the sized form at N = 4
            L.check(a._lib.g2048_sized_search_choose(4, args[0], args[1], m, L.ptr(acts4), None, a._stream))
            assert torch.equal(acts4, actions)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(actions[:m].cpu().numpy(), act)
        assert bool((actions[m:] == S8).all()) and bool((qbuf[m:] == S64).all())
        if with_q:
            np.testing.assert_array_equal(qbuf[:m].cpu().numpy(), q)
        else:
            assert bool((qbuf == S64).all())


# ------------------------------------------------------------------------------- replay with refills and suspensions
def _row_boards(b, size):
    """The valid rows of a batch: (planes [W, rows] uint64, actions [rows], valid mask [T, n])."""
    lens = b.lengths.cpu().numpy().astype(np.int64)
    acts = b.actions.cpu().numpy()
    valid = np.arange(acts.shape[0])[:, None] < lens[None, :]
    boards = b.boards.cpu().numpy().view(np.uint64)
    planes = boards[:, valid] if size != 4 else boards[valid][None]
    return planes, acts[valid], valid


def _replay(case, depth, config, max_steps, size, n, base, cap0=16, budget=16):
    if case not in _done:
        env = dict(RR.CONFIGS[config], max_steps=max_steps)
        a = _agent(env, size=size, cap0=cap0, budget=budget, max_workgroups=1)
        es = np.arange(base, base + n, dtype=np.int64)
        ps = es + 10 ** 9
        pol = _policy(depth)
        b = a.rollout_batch(es, ps, action_gen=pol)
        assert a.last_paths()["rollout"] == ROLL[size != 4] and b.probs is None
        c = RR.replay_4x4(b, env, es) if size == 4 else RR.replay_sized(b, size, env, es)
        assert c["rows"] == int(b.lengths.sum())
        # every row's action == the host build of the player on that row's board, in both games at 4 x 4
        planes, acts, valid = _row_boards(b, size)
        want, q = native_choose(size, size == 4, depth, planes)
        np.testing.assert_array_equal(acts, want)
        if size == 4:
            np.testing.assert_array_equal(native_choose(4, False, depth, planes)[0], want)
        other, _ = native_choose(size, size == 4, 1 - depth if depth < 2 else 1, planes)
        nvalid = (q >= 0).sum(axis=1)
        assert (nvalid >= 1).all()
        c["ties"] = int((((q == q.max(axis=1, keepdims=True)) & (q >= 0)).sum(axis=1) > 1).sum())
        c["depth_differs"] = int((other != want).sum())
        first_valid = np.argmax(q >= 0, axis=1)                                  # PriorityPolicy.URDL's choice
        c["priority_differs"] = int((first_valid != want).sum())
        print(case, {k: v for k, v in c.items() if k != "masks"}, "T", b.T, "median length",
              int(b.lengths.median()), flush=True)
        _done[case] = (a, es, ps, pol, b, c)
    return _done[case]


# (size, depth, config, max_steps, n): one workgroup is G2048_SCRIPT_BLOCK = 256 lanes; 229 more episodes make lanes
# take a second one from the queue
REFILL_CASES = [(4, 0, "R-raw-mask", None, 256 + 229), (3, 1, "R-raw-mask", None, 256 + 229),
                (3, 1, "R-log2-nomask", None, 256 + 229), (3, 2, "R-raw-mask", None, 64)]


def _refill_case(size, depth, config, max_steps, n):
    case = f"N{size}-d{depth}-{config}-{max_steps}"
    base = 500_000 + 1000 * REFILL_CASES.index((size, depth, config, max_steps, n))
    return _replay(case, depth, config, max_steps, size, n, base)


@pytest.mark.parametrize("size,depth,config,max_steps,n", REFILL_CASES,
                         ids=[f"N{c[0]}-d{c[1]}-{c[2]}" for c in REFILL_CASES])
def test_refilled_lanes_and_suspensions_replay(size, depth, config, max_steps, n):
    from rl2048_amd import _lib as L

    a, es, ps, pol, b, c = _refill_case(size, depth, config, max_steps, n)
    assert b.n == n and int(b.lengths.min()) >= 1 and (n == 64 or n > L.SCRIPT_BLOCK)
    assert c["terminated"] == n and c["truncated"] == 0 and c["merges"] > 0 and c["bonus"] > 0
    assert c["invalid"] == 0                                   # also with the mask off
    assert b.T > 2 * 16, "no episode was suspended twice: the test proves less than it says"
    assert c["ties"] > 0, "no row with a tie between two valid actions"
    assert c["depth_differs"] > 0, "no row where another depth chooses otherwise"
    assert c["priority_differs"] > 0, "no row where PriorityPolicy.URDL chooses otherwise"


@pytest.mark.parametrize("budget", [16, 256])
@pytest.mark.parametrize("size,depth,config,max_steps,n", REFILL_CASES,
                         ids=[f"N{c[0]}-d{c[1]}-{c[2]}" for c in REFILL_CASES])
def test_score_only_equals_rollout(size, depth, config, max_steps, n, budget):
    a, es, ps, pol, b, c = _refill_case(size, depth, config, max_steps, n)
    keep = a.search_step_budget
    try:
        a.search_step_budget = budget
        ev = a.evaluate_batch(es, ps, action_gen=pol)
    finally:
        a.search_step_budget = keep
    assert a.last_paths()["eval"] == EVAL[size != 4]
    _same_eval(ev, b)


# ------------------------------------------------------------------------------------------------ direct C calls
@pytest.mark.parametrize("size", [4, 3])
def test_direct_calls_on_a_strict_subset(size):
    """g2048_*search_rollout and g2048_*search_eval on 41 of 96 episodes, with cap / step_limit = the median length of
    those 41 (about half of them end in the call, half are suspended): what the call does not list, and everything past
    the buffers' used part, keeps its sentinel; the policy stream buffers stay byte for byte."""
    from rl2048_amd import _lib as L
    from rl2048_amd.config import env_cfg_struct

    n, pad, depth = 96, 7, 1
    W = SR.words(size)
    env = dict(RR.CONFIGS["R-raw-mask"], max_steps=None)
    a = _agent(env, size=size)
    lib, stream = a._lib, a._stream
    es = np.arange(600_000, 600_000 + n, dtype=np.int64)
    ps = es + 10 ** 9
    order_np = np.random.default_rng(5).permutation(n)[:41].astype(np.int32)
    listed = np.zeros(n, dtype=bool)
    listed[order_np] = True
    ref = a.rollout_batch(es, ps, action_gen=_policy(depth))       # the episodes' true course (replayed above)
    rlen = ref.lengths.cpu().numpy()
    cap = int(np.median(rlen[listed]))
    assert cap > 16 and int(rlen[listed].min()) < cap < int(rlen[listed].max())
    rboards = ref.boards.cpu().numpy().reshape(W, -1, n)            # [W, T, n]
    rfinal = ref.final_boards.cpu().numpy().reshape(W, n)
    cfg = env_cfg_struct(a.env_config)
    sp = _policy(depth)._search()
    for form in ("rollout", "eval"):
        seeds = [torch.from_numpy(x.view(np.int64).copy()).to(DEV) for x in (es, ps)]
        streams = []
        for sd in seeds:
            st, inc, buf = (torch.empty(k, dtype=torch.int64, device=DEV) for k in (2 * n, 2 * n, n))
            L.check(lib.g2048_seed_pcg64(L.ptr(sd), L.ptr(st), L.ptr(inc), L.ptr(buf), n, stream))
            streams += [st, inc, buf]
        before = [t.clone() for t in streams]
        S8, S32, S64 = 0xA5, -77, -0x5A5A5A5A5A5A5A5B
        boards = torch.full((W, cap + 1, n), S64, dtype=torch.int64, device=DEV)
        actions = torch.full((cap + 1, n), S8, dtype=torch.uint8, device=DEV)
        rewards = torch.full((cap + 1, n), -123.25, dtype=torch.float64, device=DEV)
        flags = torch.full((cap + 1, n), S8, dtype=torch.uint8, device=DEV)
        lengths = torch.full((n + pad,), S32, dtype=torch.int32, device=DEV)
        totals = torch.full((n + pad,), -123.25, dtype=torch.float64, device=DEV)
        max_e = torch.full((n + pad,), S8, dtype=torch.uint8, device=DEV)
        final = torch.full((W + 1, n), S64, dtype=torch.int64, device=DEV)          # one plane more than the call uses
        sus_board = torch.full((W + 1, n), S64, dtype=torch.int64, device=DEV)
        sus_meta = torch.full((3 * n + pad,), S32, dtype=torch.int32, device=DEV)
        sus_total = torch.full((n + pad,), -123.25, dtype=torch.float64, device=DEV)
        sus_list = torch.full((n + pad,), S32, dtype=torch.int32, device=DEV)
        sus_count = torch.zeros(1, dtype=torch.int32, device=DEV)
        queue = torch.zeros(1, dtype=torch.int32, device=DEV)
        order = torch.from_numpy(order_np).to(DEV)
        sus = L.Suspend(*[L.ptr(t) for t in (sus_board, sus_meta, sus_total, sus_list, sus_count)])
        head = ((size,) if size != 4 else ()) + (
            ctypes.byref(sp), ctypes.byref(cfg), *[L.ptr(t) for t in streams], L.ptr(queue), L.ptr(order),
            len(order_np), 0, ctypes.byref(sus), n, cap)
        if form == "rollout":
            traj = L.Traj(*[L.ptr(t) for t in (boards, actions, rewards, flags, None, lengths, totals, max_e, final)])
            if size != 4:       # the planes' stride: the buffer's own (cap + 1 rows), more than cap * n
                L.check(lib.g2048_sized_search_rollout(*head, ctypes.byref(traj), (cap + 1) * n, 1, stream))
            else:
                L.check(lib.g2048_search_rollout(*head, ctypes.byref(traj), 1, stream))
        else:
            out = L.EvalOut(*[L.ptr(t) for t in (lengths, totals, max_e, final)])
            L.check((lib.g2048_sized_search_eval if size != 4 else lib.g2048_search_eval)(
                *head, ctypes.byref(out), 1, stream))
        torch.cuda.synchronize()
        ended = listed & (rlen <= cap)
        susp = listed & (rlen > cap)
        k = int(sus_count.item())
        assert k == int(susp.sum()) and 0 < k < len(order_np) and int(queue.item()) >= len(order_np)
        got_list = sus_list.cpu().numpy()
        assert sorted(got_list[:k].tolist()) == np.nonzero(susp)[0].tolist() and (got_list[k:] == S32).all()
        # per-episode outputs: written for the listed episodes that ended, sentinel elsewhere and in the tail
        ln, tt, me, fb = (t.cpu().numpy() for t in (lengths, totals, max_e, final))
        e_idx, o_idx = np.nonzero(ended)[0], np.nonzero(~np.concatenate([ended, np.zeros(pad, bool)]))[0]
        np.testing.assert_array_equal(ln[e_idx], rlen[e_idx])
        np.testing.assert_array_equal(tt[e_idx].view(np.uint64), ref.total_reward.cpu().numpy()[e_idx].view(np.uint64))
        np.testing.assert_array_equal(1 << me[e_idx].astype(np.int64), ref.max_tile.cpu().numpy()[e_idx])
        np.testing.assert_array_equal(fb[:W, e_idx], rfinal[:, e_idx])
        assert (ln[o_idx] == S32).all() and (tt[o_idx] == -123.25).all() and (me[o_idx] == S8).all()
        assert (fb[:W, ~ended] == S64).all() and (fb[W] == S64).all()
        # suspend state: only the suspended episodes'
        sb, sm, stot = sus_board.cpu().numpy(), sus_meta.cpu().numpy(), sus_total.cpu().numpy()
        s_idx = np.nonzero(susp)[0]
        not_s = np.nonzero(~np.concatenate([susp, np.zeros(pad, bool)]))[0]
        assert (sb[:W, ~susp] == S64).all() and (sb[W] == S64).all()
        assert (stot[not_s] == -123.25).all() and (sm[3 * n:] == S32).all()
        assert (sm[:3 * n].reshape(n, 3)[~susp] == S32).all()
        np.testing.assert_array_equal(sm[:3 * n].reshape(n, 3)[s_idx][:, :2], np.full((k, 2), cap))
        np.testing.assert_array_equal(sb[:W, s_idx], rboards[:, cap, s_idx])         # the board before step `cap`
        tot_cap = np.zeros(n)
        rr = ref.rewards.cpu().numpy()
        for t in range(cap):
            tot_cap = tot_cap + rr[t]
        np.testing.assert_array_equal(stot[s_idx].view(np.uint64), tot_cap[s_idx].view(np.uint64))
        # rows
        bo, ac, rw, fl = (t.cpu().numpy() for t in (boards, actions, rewards, flags))
        if form == "rollout":
            racts = ref.actions.cpu().numpy()
            for i in range(n):
                T = min(int(rlen[i]), cap) if listed[i] else 0
                np.testing.assert_array_equal(bo[:, :T, i], rboards[:, :T, i])
                np.testing.assert_array_equal(ac[:T, i], racts[:T, i])
                np.testing.assert_array_equal(rw[:T, i].view(np.uint64), rr[:T, i].view(np.uint64))
                assert (bo[:, T:, i] == S64).all() and (ac[T:, i] == S8).all() and (rw[T:, i] == -123.25).all()
                assert (fl[T:, i] == S8).all() and (fl[:T, i] != S8).all()
        else:
            assert (bo == S64).all() and (ac == S8).all() and (rw == -123.25).all() and (fl == S8).all()
        # streams: inc never changes; env streams change only for suspended episodes; the policy's never
        assert torch.equal(streams[1], before[1]) and torch.equal(streams[4], before[4])
        est, est0 = streams[0].cpu().numpy().reshape(n, 2), before[0].cpu().numpy().reshape(n, 2)
        assert (est[~susp] == est0[~susp]).all() and (est[susp] != est0[susp]).any(axis=1).all()
        assert torch.equal(streams[3], before[3]) and torch.equal(streams[5], before[5])


# ---------------------------------------------------------------------------------------------------- run_episode
def test_run_episode_device_path_equals_host_path():
    env = dict(RR.CONFIGS["R-raw-mask"], obs_mode="log2", max_steps=None)
    a = _agent(env, size=3, max_workgroups=0)
    pol = _policy(1)
    dev = a.run_episode(21, 26, action_gen=pol)
    assert a.last_paths()["rollout"] == ROLL[True]
    a._paths.pop("rollout")
    host = a.run_episode(21, 26, action_gen=lambda state, mask: pol(state, mask))     # a plain callable: the host loop
    assert "rollout" not in a.last_paths()
    assert sorted(dev) == sorted(host) == ["actions", "max_tile", "obs", "rewards", "states", "total_reward"]
    assert dev["actions"] == host["actions"] and len(dev["actions"]) > 20
    assert np.array_equal(np.array(dev["rewards"]).view(np.uint64), np.array(host["rewards"]).view(np.uint64))
    assert dev["states"] == host["states"]
    assert np.float64(dev["total_reward"]).view(np.uint64) == np.float64(host["total_reward"]).view(np.uint64)
    assert dev["max_tile"] == host["max_tile"] and len(dev["obs"]) == len(host["obs"])
    for x, y in zip(dev["obs"], host["obs"]):
        assert sorted(x) == sorted(y) == ["action_mask", "board"]
        for key in x:
            xa, ya = np.asarray(x[key]), np.asarray(y[key])
            assert xa.shape == ya.shape and xa.dtype == ya.dtype and np.array_equal(xa, ya), key


# -------------------------------------------------------------------------------------------------------- updates
@pytest.mark.parametrize("size", [4, 3])
def test_update_from_a_search_teacher_batch(size):
    """update_from_batch on a teacher batch runs on the default path, and on the general gradient path (the fp32 GEMM
    path, use_fused_grad off) it equals update_batch -- reference-format trajectories with their obs from the host,
    which always takes that path -- on the same trajectories from the same initial parameters: gradients and the
    parameters after the step, with ==."""
    env = dict(obs_mode="log2", obs_log2_scale=0.0625, reward_mode="log2", base_reward_scale=0.5, max_steps=40)
    kw = dict(gamma=0.99, learning_rate=1e-2, baseline_mode="batch")
    d, a, b = (_agent(env, size=size, cap0=64, max_workgroups=0, **kw) for _ in range(3))
    es = np.arange(8, dtype=np.int64) + 700_000
    batch = a.rollout_batch(es, es + 5, action_gen=_policy(1))
    assert int(batch.lengths.sum()) > 100
    before = [p.clone() for p in d.params["W"] + d.params["b"]]
    stats = d.update_from_batch(batch)                              # the default path (fused kernels where they apply)
    assert np.isfinite(stats["actor_grad_norm"]) and stats["actor_grad_norm"] > 0
    assert any(not torch.equal(x, y) for x, y in zip(before, d.params["W"] + d.params["b"]))
    a.use_fused_grad = b.use_fused_grad = False
    a.update_from_batch(batch)
    b.update_batch(b.trajectories_from_batch(batch, with_states=False))
    assert a.last_paths().get("actor_grad") == b.last_paths().get("actor_grad")
    for ga, gb in zip(a.last_grads["actor"], b.last_grads["actor"]):
        assert torch.equal(ga, gb)
    after = a.params["W"] + a.params["b"]
    assert any(not torch.equal(x, y) for x, y in zip(before, after))
    for x, y in zip(after, b.params["W"] + b.params["b"]):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------ the runner
def test_runner_evaluation_loop_with_the_search_player():
    from rl2048_amd import PriorityPolicy, runner

    a = _agent(dict(max_steps=None), cap0=256, budget=256, max_workgroups=0)
    cfg = dict(num_episodes=128, env_base_seed=31, policy_base_seed=32, use_greedy=True)
    pol = _policy(0)
    s0 = runner.evaluation_loop(a, cfg, action_gen=pol)
    assert a.last_paths()["rollout"] == ROLL[False]
    s1 = runner.evaluation_loop(a, cfg, score_only=True, action_gen=pol)
    assert a.last_paths()["eval"] == EVAL[False]
    assert s0 == s1 and s0["episodes"] == 128
    # a lookahead player beats the priority baseline on the same seeds
    s2 = runner.evaluation_loop(a, cfg, score_only=True, action_gen=PriorityPolicy(PriorityPolicy.URLD))
    assert s0["avg_reward"] > s2["avg_reward"]
