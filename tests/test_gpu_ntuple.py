"""GPU: the n-tuple value network (rollout_batch / evaluate_batch / run_episode / evaluation_loop with action_gen =
NTuplePolicy, agent.ntuple_actions, NTupleNetwork.values, agent.ntuple_update; g2048_*ntuple_* of
include/g2048_ntuple.h).

* the fixture episodes (tests/golden/ntuple.npz: the real reference's run_episode with the player as action_gen) row
  for row, evaluate_batch == rollout_batch, last_paths() names the new kernels;
* ntuple_actions, values and the direct *_ntuple_choose / *_ntuple_values calls on the fixture boards (294 boards: more
  than one workgroup, no multiple of 64), sentinels past the outputs, q = NULL, the sized form at N = 4;
* refilled lanes and repeated suspensions (one workgroup, first capacity 16): every row replays in the CPU oracles
  (tests/rollout_replay.py) and every row's action equals the host build of the player (tests/native/ntuple_host.cpp)
  on that row's board, mask on and off; the score-only form at budgets 16 and 256;
* the TD(0) update: the fixture cases, the refill batches (thousands of concurrent adds on the hot entries) against the
  host build on every weight, and the same call twice from the same start;
* a closed loop of rollout -> update -> evaluate against the same loop driven through the host build;
* run_episode's device path == its host path driven by the Python callable; the runner's evaluation_loop; a teacher
  batch through update_from_batch.

Every comparison is ==.
"""
import ctypes

import numpy as np
import pytest
import torch

import ntuple_ref as NR
import rollout_replay as RR
import sized_ref as SR
from ntuple_ref import BOARD_SIZES, INVALID

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROLL = {False: "g2048_ntuple_rollout (persistent launches, one episode per lane played by an n-tuple network, suspended "
               "episodes resumed)",
        True: "g2048_sized_ntuple_rollout (persistent launches, one episode per lane played by an n-tuple network, "
              "suspended episodes resumed)"}
EVAL = {False: "g2048_ntuple_eval (persistent launches, one episode per lane played by an n-tuple network, no "
               "trajectory rows, suspended episodes resumed)",
        True: "g2048_sized_ntuple_eval (persistent launches, one episode per lane played by an n-tuple network, no "
              "trajectory rows, suspended episodes resumed)"}
_done: dict = {}            # case id -> (agent, env seeds, policy seeds, policy, batch, counts): computed once
_nets: dict = {}


@pytest.fixture(scope="module")
def gold():
    return NR.golden()


def net_of(size):
    """The device network with the fixture's hash weights (shared: tests that train work on a copy)."""
    if size not in _nets:
        _nets[size] = NR.make_net(size, device=DEV)
    return _nets[size]


def _agent(env: dict, size=4, cap0=16, budget=16, max_workgroups=1, **agent_kw):
    from rl2048_amd import Game2048EnvConfig
    from rl2048_amd.agent import ReinforceAgent, ReinforceAgentConfig
    from rl2048_amd.mlp import MLPConfig

    a = ReinforceAgent(Game2048EnvConfig(size=size, **env), MLPConfig(hidden_sizes=[8], activation="ReLU"),
                       ReinforceAgentConfig(model_seed=3, **agent_kw), device=DEV)
    a.ntuple_rollout_cap0, a.ntuple_step_budget, a.ntuple_max_workgroups = cap0, budget, max_workgroups
    return a


def _policy(size, depth, net=None):
    from rl2048_amd import NTuplePolicy

    return NTuplePolicy(net_of(size) if net is None else net, depth)


def _same_eval(ev, b):
    assert ev.lengths.dtype == b.lengths.dtype and torch.equal(ev.lengths, b.lengths)
    assert ev.total_reward.dtype == torch.float64
    assert torch.equal(ev.total_reward.view(torch.int64), b.total_reward.view(torch.int64))     # fp64 totals by bits
    assert ev.max_tile.dtype == b.max_tile.dtype and torch.equal(ev.max_tile, b.max_tile)
    assert ev.final_boards.shape == b.final_boards.shape and torch.equal(ev.final_boards, b.final_boards)


# ------------------------------------------------------------------------------------------ the reference's episodes
@pytest.mark.parametrize("c", range(7))
def test_fixture_episodes(gold, c):
    case = NR.ep_cases()[c]
    size, depth = case["size"], case["depth"]
    a = _agent(case["env"], size=size, cap0=16, max_workgroups=0)
    P = f"e{c}_"
    lens = gold[P + "length"]
    start = np.concatenate([[0], np.cumsum(lens)])
    es, ps = gold[P + "env_seed"].astype(np.int64), gold[P + "policy_seed"].astype(np.int64)
    b = a.rollout_batch(es, ps, action_gen=_policy(size, depth))
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
    _same_eval(a.evaluate_batch(es, ps, action_gen=_policy(size, depth)), b)
    assert a.last_paths()["eval"] == EVAL[size != 4]


# ------------------------------------------------------------------------------------------------- single choices
@pytest.mark.parametrize("size", BOARD_SIZES)
def test_actions_values_and_direct_calls_on_the_fixture_boards(gold, size):
    from rl2048_amd import _lib as L

    e = gold[f"b{size}_boards"]
    m = len(e)
    assert m % 64 != 0 and m > L.SCRIPT_BLOCK
    planes = torch.from_numpy(SR.pack_planes(e, size)).to(DEV)                   # [W, m]
    boards = planes if size != 4 else planes[0]
    a = _agent(dict(max_steps=None), size=size)
    net = net_of(size)
    np.testing.assert_array_equal(net.values(boards).cpu().numpy(), gold[f"b{size}_v"])
    i1 = gold[f"b{size}_i1"]
    for depth, sel in ((0, np.arange(m)), (1, i1)):
        pol = _policy(size, depth)
        q, act = gold[f"b{size}_q{depth}"], gold[f"b{size}_a{depth}"]
        sub = planes[:, torch.from_numpy(sel).to(DEV)].contiguous()
        k = len(sel)
        got_a, got_q = a.ntuple_actions(sub if size != 4 else sub[0], pol)
        assert got_a.dtype == torch.uint8 and got_q.dtype == torch.int64 and got_a.shape == (k,) and got_q.shape == (k, 4)
        np.testing.assert_array_equal(got_q.cpu().numpy(), q)
        np.testing.assert_array_equal(got_a.cpu().numpy(), act)
        assert "ntuple_choose" in a.last_paths()["ntuple_actions"]
        # any leading shape: TrajectoryBatch.boards as it is
        h = k // 2
        shaped = sub[:, :2 * h].reshape(-1, 2, h) if size != 4 else sub[0, :2 * h].reshape(2, h)
        sa, sq = a.ntuple_actions(shaped, pol)
        assert sa.shape == (2, h) and sq.shape == (2, h, 4)
        np.testing.assert_array_equal(sa.cpu().numpy().reshape(-1), act[:2 * h])
        np.testing.assert_array_equal(sq.cpu().numpy().reshape(-1, 4), q[:2 * h])
        # the direct calls: sentinels past the outputs' used part, q = NULL
        pad, S8, S64 = 5, 0xA5, -0x5A5A5A5A5A5A5A5B
        d = pol._ntuple()
        for with_q in (True, False):
            actions = torch.full((k + pad,), S8, dtype=torch.uint8, device=DEV)
            qbuf = torch.full((k + pad, 4), S64, dtype=torch.int64, device=DEV)
            args = (ctypes.byref(d), L.ptr(sub), k, L.ptr(actions), L.ptr(qbuf) if with_q else None, a._stream)
            if size != 4:
                L.check(a._lib.g2048_sized_ntuple_choose(size, *args))
            else:
                L.check(a._lib.g2048_ntuple_choose(*args))
                acts4 = torch.full((k + pad,), S8, dtype=torch.uint8, device=DEV)     # ... and the sized form at N = 4
                L.check(a._lib.g2048_sized_ntuple_choose(4, args[0], args[1], k, L.ptr(acts4), None, a._stream))
                assert torch.equal(acts4, actions)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(actions[:k].cpu().numpy(), act)
            assert bool((actions[k:] == S8).all()) and bool((qbuf[k:] == S64).all())
            if with_q:
                np.testing.assert_array_equal(qbuf[:k].cpu().numpy(), q)
            else:
                assert bool((qbuf == S64).all())
    # values, directly
    vals = torch.full((m + 5,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=DEV)
    d = net._descriptor()
    if size != 4:
        L.check(a._lib.g2048_sized_ntuple_values(size, ctypes.byref(d), L.ptr(planes), m, L.ptr(vals), a._stream))
    else:
        L.check(a._lib.g2048_ntuple_values(ctypes.byref(d), L.ptr(planes), m, L.ptr(vals), a._stream))
        v4 = torch.empty(m, dtype=torch.int64, device=DEV)
        L.check(a._lib.g2048_sized_ntuple_values(4, ctypes.byref(d), L.ptr(planes), m, L.ptr(v4), a._stream))
        assert torch.equal(v4, vals[:m])
    np.testing.assert_array_equal(vals[:m].cpu().numpy(), gold[f"b{size}_v"])
    assert bool((vals[m:] == -0x5A5A5A5A5A5A5A5B).all())


# ------------------------------------------------------------------------------- replay with refills and suspensions
def _row_boards(b, size):
    """The valid rows of a batch: (planes [W, rows] uint64, actions [rows], valid mask [T, n])."""
    lens = b.lengths.cpu().numpy().astype(np.int64)
    acts = b.actions.cpu().numpy()
    valid = np.arange(acts.shape[0])[:, None] < lens[None, :]
    boards = b.boards.cpu().numpy().view(np.uint64)
    planes = boards[:, valid] if size != 4 else boards[valid][None]
    return planes, acts[valid], valid


# (size, depth, config, n): one workgroup is G2048_SCRIPT_BLOCK = 256 lanes.  At depth 0 the 229 episodes past it make
# lanes take a second one from the queue (refill).  The depth-1 cases, n = 64 + 37, fit the workgroup: no lane refills;
# they cover a ragged second wave and repeated suspension and resume only.
REFILL_CASES = [(4, 0, "R-raw-mask", 256 + 229), (4, 0, "R-log2-nomask", 256 + 229), (3, 1, "R-raw-mask", 64 + 37),
                (3, 1, "R-log2-nomask", 64 + 37)]


def _refill_case(size, depth, config, n):
    case = f"N{size}-d{depth}-{config}"
    if case not in _done:
        base = 800_000 + 1000 * REFILL_CASES.index((size, depth, config, n))
        env = dict(RR.CONFIGS[config], max_steps=None)
        a = _agent(env, size=size, cap0=16, budget=16, max_workgroups=1)
        es = np.arange(base, base + n, dtype=np.int64)
        ps = es + 10 ** 9
        pol = _policy(size, depth)
        b = a.rollout_batch(es, ps, action_gen=pol)
        assert a.last_paths()["rollout"] == ROLL[size != 4] and b.probs is None
        c = RR.replay_4x4(b, env, es) if size == 4 else RR.replay_sized(b, size, env, es)
        assert c["rows"] == int(b.lengths.sum())
        # every row's action == the host build of the player on that row's board, in both games at 4 x 4
        planes, acts, valid = _row_boards(b, size)
        want, q = NR.host_choose(pol.network, size == 4, depth, planes)
        np.testing.assert_array_equal(acts, want)
        if size == 4:
            np.testing.assert_array_equal(NR.host_choose(pol.network, False, depth, planes)[0], want)
        ok = q != INVALID
        assert (ok.sum(axis=1) >= 1).all()
        best = np.where(ok, q, INVALID).max(axis=1)
        c["ties"] = int((((q == best[:, None]) & ok).sum(axis=1) > 1).sum())
        print(case, {k: v for k, v in c.items() if k != "masks"}, "T", b.T, "median length",
              int(b.lengths.median()), flush=True)
        _done[case] = (a, es, ps, pol, b, c)
    return _done[case]


@pytest.mark.parametrize("size,depth,config,n", REFILL_CASES, ids=[f"N{c[0]}-d{c[1]}-{c[2]}" for c in REFILL_CASES])
def test_refilled_lanes_and_suspensions_replay(size, depth, config, n):
    a, es, ps, pol, b, c = _refill_case(size, depth, config, n)
    assert b.n == n and int(b.lengths.min()) >= 1
    assert c["terminated"] == n and c["truncated"] == 0 and c["merges"] > 0
    assert c["invalid"] == 0                                   # also with the mask off
    assert b.T > 32, "no episode was suspended twice: the test proves less than it says"
    assert c["ties"] > 0, "no row with a tie between two valid actions"


@pytest.mark.parametrize("budget", [16, 256])
@pytest.mark.parametrize("size,depth,config,n", REFILL_CASES, ids=[f"N{c[0]}-d{c[1]}-{c[2]}" for c in REFILL_CASES])
def test_score_only_equals_rollout(size, depth, config, n, budget):
    a, es, ps, pol, b, c = _refill_case(size, depth, config, n)
    keep = a.ntuple_step_budget
    try:
        a.ntuple_step_budget = budget
        ev = a.evaluate_batch(es, ps, action_gen=pol)
    finally:
        a.ntuple_step_budget = keep
    assert a.last_paths()["eval"] == EVAL[size != 4]
    _same_eval(ev, b)


# ---------------------------------------------------------------------------------------------------------- TD
def _batch_of(planes, actions, flags, lengths, size):
    """A TrajectoryBatch on the device from numpy rows (what the update reads; the rest is filled with zeros)."""
    from rl2048_amd.agent import TrajectoryBatch

    T, n = actions.shape
    p = torch.from_numpy(np.ascontiguousarray(planes).view(np.int64).reshape(-1, T, n)).to(DEV)
    return TrajectoryBatch(boards=p if size != 4 else p[0].contiguous(), actions=torch.from_numpy(actions).to(DEV),
                           rewards=torch.zeros(T, n, dtype=torch.float64, device=DEV),
                           flags=torch.from_numpy(flags).to(DEV), lengths=torch.from_numpy(lengths).to(DEV),
                           total_reward=torch.zeros(n, dtype=torch.float64, device=DEV),
                           max_tile=torch.zeros(n, dtype=torch.int64, device=DEV),
                           final_boards=torch.zeros(n, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize("size", [3, 4])
def test_td_fixture_cases(gold, size):
    from rl2048_amd import _lib as L

    net = NR.make_net(size, device=DEV)
    before = net.host_weights().copy()
    planes, actions, flags, lengths = NR.td_case(size)
    lr_num, lr_shift = (int(x) for x in gold[f"td{size}_lr"])
    want, rows, abs_delta = NR.td_expected(size, before)
    a = _agent(dict(max_steps=None), size=size)
    batch = _batch_of(planes, actions, flags, lengths, size)
    import dataclasses
    wrong = batch.boards[0] if size != 4 else batch.boards[None]      # the other game's board layout
    with pytest.raises(ValueError, match="batch.boards"):
        a.ntuple_update(dataclasses.replace(batch, boards=wrong), net, lr_num, lr_shift)
    with pytest.raises(ValueError, match="the batch is on"):
        a.ntuple_update(dataclasses.replace(batch, flags=batch.flags.cpu()), net, lr_num, lr_shift)
    assert "ntuple_update" not in a.last_paths() and np.array_equal(net.weights.cpu().numpy(), before)
    st = a.ntuple_update(batch, net, lr_num, lr_shift)
    assert st == {"rows": rows, "abs_delta": abs_delta, "path": a.last_paths()["ntuple_update"]}
    assert ("g2048_sized_ntuple_td_update" if size != 4 else "g2048_ntuple_td_update") in st["path"]
    np.testing.assert_array_equal(net.weights.cpu().numpy(), want)
    np.testing.assert_array_equal(net.host_weights(), want)         # the Python statement sees the new weights
    if size == 4:       # the sized form at N = 4, called directly
        net.load_state_dict(dict(net.state_dict(), weights=before))
        T, n = actions.shape
        scratch = torch.empty(2 * T * n, dtype=torch.int64, device=DEV)
        stats = torch.full((3,), -7, dtype=torch.int64, device=DEV)
        d = net._descriptor()
        L.check(a._lib.g2048_sized_ntuple_td_update(4, ctypes.byref(d), L.ptr(batch.boards), T * n, L.ptr(batch.actions),
                                                    L.ptr(batch.flags), L.ptr(batch.lengths), n, T, lr_num, lr_shift,
                                                    L.ptr(scratch), L.ptr(stats), a._stream))
        assert stats.tolist() == [rows, abs_delta, -7]
        np.testing.assert_array_equal(net.weights.cpu().numpy(), want)


@pytest.mark.parametrize("size,depth,config,n", REFILL_CASES[::2], ids=[f"N{c[0]}-d{c[1]}" for c in REFILL_CASES[::2]])
def test_td_on_a_large_batch_equals_the_host_build(size, depth, config, n):
    a, es, ps, pol, b, c = _refill_case(size, depth, config, n)
    net = NR.make_net(size, device=DEV)
    before = net.host_weights().copy()
    W = SR.words(size)
    planes = b.boards.cpu().numpy().reshape(W, b.T, n)
    want, rows, abs_delta = NR.host_td(net, size == 4, before, planes, b.actions.cpu().numpy(), b.flags.cpu().numpy(),
                                       b.lengths.cpu().numpy(), 1, 6)
    assert rows == int(b.lengths.sum())                            # every episode terminated: every row counts
    # the hot entries (index 0 of a table: all cells of the tuple empty) take an add from most of the rows
    st = a.ntuple_update(b, net, 1, 6)
    assert (st["rows"], st["abs_delta"]) == (rows, abs_delta) and rows > 2000
    got = net.weights.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    assert int((got != before).sum()) > 1000
    # the same call from the same start gives the same weights
    net.load_state_dict(dict(net.state_dict(), weights=before))
    st2 = a.ntuple_update(b, net, 1, 6)
    assert (st2["rows"], st2["abs_delta"]) == (rows, abs_delta)
    assert torch.equal(net.weights, torch.from_numpy(want).to(DEV))


# --------------------------------------------------------------------------------------------------- closed loop
@pytest.mark.parametrize("size,max_steps", [(3, None), (4, 64)])
def test_closed_loop_equals_the_host_loop(size, max_steps):
    """3 iterations of rollout -> update -> evaluate on 64 episodes: the weights after the last update and every
    iteration's evaluation totals equal the same loop driven through the host build."""
    env = dict(RR.CONFIGS["R-raw-mask"], max_steps=max_steps)
    a = _agent(env, size=size, cap0=32, budget=64, max_workgroups=0)
    net = NR.make_net(size, device=DEV)
    pol = _policy(size, 0, net)
    w = net.host_weights().copy()
    ev_e = np.arange(64, dtype=np.int64) + 910_000
    for it in range(3):
        es = np.arange(64, dtype=np.int64) + 900_000 + 100 * it
        b = a.rollout_batch(es, es + 7, action_gen=pol)
        st = a.ntuple_update(b, net, 1, 4)
        ev = a.evaluate_batch(ev_e, ev_e + 7, action_gen=pol)
        planes, actions, flags, lengths, _ = NR.host_rollout(net, size == 4, 0, env, es, es + 7, weights=w)
        np.testing.assert_array_equal(b.lengths.cpu().numpy(), lengths)
        w, rows, abs_delta = NR.host_td(net, size == 4, w, planes, actions, flags, lengths, 1, 4)
        assert (st["rows"], st["abs_delta"]) == (rows, abs_delta)
        *_, hl, ht = NR.host_rollout(net, size == 4, 0, env, ev_e, ev_e + 7, weights=w)
        np.testing.assert_array_equal(ev.lengths.cpu().numpy(), hl)
        np.testing.assert_array_equal(ev.total_reward.cpu().numpy().view(np.uint64), ht.view(np.uint64))
    np.testing.assert_array_equal(net.weights.cpu().numpy(), w)
    assert int((w != NR.make_net(size).host_weights()).sum()) > 1000


# ---------------------------------------------------------------------------------------------------- run_episode
def test_run_episode_device_path_equals_host_path():
    env = dict(RR.CONFIGS["R-raw-mask"], obs_mode="log2", max_steps=None)
    a = _agent(env, size=3, max_workgroups=0)
    pol = _policy(3, 1)
    dev = a.run_episode(21, 26, action_gen=pol)
    assert a.last_paths()["rollout"] == ROLL[True]
    a._paths.pop("rollout")
    host = a.run_episode(21, 26, action_gen=lambda state, mask: pol(state, mask))     # a plain callable: the host loop
    assert "rollout" not in a.last_paths()
    assert sorted(dev) == sorted(host) == ["actions", "max_tile", "obs", "rewards", "states", "total_reward"]
    assert dev["actions"] == host["actions"] and len(dev["actions"]) > 10
    assert np.array_equal(np.array(dev["rewards"]).view(np.uint64), np.array(host["rewards"]).view(np.uint64))
    assert dev["states"] == host["states"]
    assert np.float64(dev["total_reward"]).view(np.uint64) == np.float64(host["total_reward"]).view(np.uint64)
    assert dev["max_tile"] == host["max_tile"] and len(dev["obs"]) == len(host["obs"])


# ------------------------------------------------------------------------------------- the runner, a teacher batch
def test_runner_evaluation_loop_with_the_ntuple_player():
    from rl2048_amd import runner

    a = _agent(dict(max_steps=None), cap0=256, budget=256, max_workgroups=0)
    cfg = dict(num_episodes=128, env_base_seed=31, policy_base_seed=32, use_greedy=True)
    pol = _policy(4, 0)
    s0 = runner.evaluation_loop(a, cfg, action_gen=pol)
    assert a.last_paths()["rollout"] == ROLL[False]
    s1 = runner.evaluation_loop(a, cfg, score_only=True, action_gen=pol)
    assert a.last_paths()["eval"] == EVAL[False]
    assert s0 == s1 and s0["episodes"] == 128


def test_update_from_an_ntuple_teacher_batch():
    env = dict(obs_mode="log2", obs_log2_scale=0.0625, reward_mode="log2", base_reward_scale=0.5, max_steps=40)
    d = _agent(env, cap0=64, max_workgroups=0, gamma=0.99, learning_rate=1e-2, baseline_mode="batch")
    es = np.arange(8, dtype=np.int64) + 700_000
    batch = d.rollout_batch(es, es + 5, action_gen=_policy(4, 0))
    assert int(batch.lengths.sum()) > 100
    before = [p.clone() for p in d.params["W"] + d.params["b"]]
    stats = d.update_from_batch(batch)
    assert np.isfinite(stats["actor_grad_norm"]) and stats["actor_grad_norm"] > 0
    assert any(not torch.equal(x, y) for x, y in zip(before, d.params["W"] + d.params["b"]))
