"""GPU: the agent and the runner on board sizes other than 4 against the real reference (tests/golden/sized_agent.npz,
written by tests/golden/make_golden_sized.py): rollout_batch == run_episode, update_from_batch / update_batch ==
update_batch, runner.training_loop == runner.py, all on the general path (hipBLASLt forward + g2048_sample +
g2048_sized_step, torch backprop) -- the fused 4 x 4 kernels are never offered a sized board.

The fixture keeps only (env_seed, policy_seed) pairs whose every sampling draw lies at least 1e-4 from every cdf
boundary (asserted by the generator and again here), so the 2e-6 agreement of the probabilities cannot flip an action
and nothing is skipped.  Tolerances are those of tests/test_gpu_ref_fixtures.py (its helpers are imported).
"""
import json
import os

import numpy as np
import pytest
import torch

import ref_fixtures as RF
from test_gpu_ref_fixtures import assert_step_matches

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
D = RF.load("sized_agent")
CASES = json.loads(str(D["agent_cases"]))


def _agent(case):
    from rl2048_amd import Game2048EnvConfig
    from rl2048_amd.agent import ReinforceAgent, ReinforceAgentConfig
    from rl2048_amd.mlp import MLPConfig

    return ReinforceAgent(Game2048EnvConfig(**case["env"]), MLPConfig(**case["mlp"]),
                          ReinforceAgentConfig(**case["agent"]), device=DEV)


def _params(ci, prefix, L):
    flat = [D[f"a{ci}_{prefix}_{j}"] for j in range(2 * L)]
    return {"W": [a.copy() for a in flat[:L]], "b": [a.copy() for a in flat[L:]]}


def _before(ci, u, L, which):
    return _params(ci, f"init_{which}" if u == 0 else f"up{u - 1}_{which}", L)


def _set(agent, params, critic=False):
    t = {k: [torch.from_numpy(a.copy()).to(DEV) for a in v] for k, v in params.items()}
    if critic:
        agent.critic_params = t
    else:
        agent.params = t
    agent._params_version += 1


def _planes(e: np.ndarray, n: int) -> np.ndarray:
    """uint8 exponents [..., N*N] -> int64 planes [W, ...]."""
    e = np.asarray(e, dtype=np.uint64)
    out = np.zeros(((n * n + 15) // 16,) + e.shape[:-1], dtype=np.uint64)
    for k in range(n * n):
        out[k >> 4] |= e[..., k] << np.uint64(4 * (k & 15))
    return out.view(np.int64)


def _exps(p: np.ndarray, n: int) -> np.ndarray:
    p = np.asarray(p).view(np.uint64)
    return np.stack([(p[k >> 4] >> np.uint64(4 * (k & 15))) & np.uint64(15) for k in range(n * n)], axis=-1).astype(np.uint8)


def _mask_of(e: np.ndarray) -> np.ndarray:
    """get_action_mask (src/game2048.py:95-99, :233-237) of a board of exponents [N, N]."""
    out = []
    for a in range(4):
        b = np.rot90(e, k=-(3 - a))
        nz = b != 0
        gap = (~nz[:, :-1] & nz[:, 1:]).any()
        eq = (nz[:, :-1] & (b[:, :-1] == b[:, 1:])).any()
        out.append(int(gap or eq))
    return np.array(out, dtype=np.int8)


def _obs(e: np.ndarray, env: dict):
    n = env["size"]
    e = e.reshape(n, n).astype(np.int64)
    if env["obs_mode"] == "onehot":
        board = np.eye(17, dtype=np.float32)[e]
    elif env["obs_mode"] == "log2":
        board = e.astype(np.float32) * np.float32(env.get("obs_log2_scale", 1.0))
    else:
        board = np.where(e > 0, np.int64(1) << e, 0).astype(np.float32)
    if env.get("use_action_mask", True):
        return {"board": board, "action_mask": _mask_of(e)}
    return board


def _trajectories(ci, u, case):
    P = f"a{ci}_up{u}_"
    out, s = [], 0
    for i, T in enumerate(D[P + "lengths"]):
        T = int(T)
        out.append({"obs": [_obs(b, case["env"]) for b in D[P + "boards"][s:s + T]],
                    "actions": [int(a) for a in D[P + "actions"][s:s + T]],
                    "rewards": [float(r) for r in D[P + "rewards"][s:s + T]],
                    "total_reward": float(D[P + "total_reward"][i]), "states": [], "max_tile": int(D[P + "max_tile"][i])})
        s += T
    return out


def _batch(ci, u, case):
    from rl2048_amd.agent import TrajectoryBatch

    P, n_size = f"a{ci}_up{u}_", case["env"]["size"]
    lens = D[P + "lengths"]
    n, T = len(lens), int(lens.max())
    ex = np.zeros((T, n, n_size * n_size), dtype=np.uint8)
    acts = np.zeros((T, n), dtype=np.uint8)
    rews = np.zeros((T, n), dtype=np.float64)
    s = 0
    for i, Ti in enumerate(lens):
        Ti = int(Ti)
        ex[:Ti, i] = D[P + "boards"][s:s + Ti]
        acts[:Ti, i] = D[P + "actions"][s:s + Ti]
        rews[:Ti, i] = D[P + "rewards"][s:s + Ti]
        s += Ti
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    W = (n_size * n_size + 15) // 16
    return TrajectoryBatch(boards=t(_planes(ex, n_size)), actions=t(acts), rewards=t(rews),
                           flags=torch.zeros(T, n, dtype=torch.uint8, device=DEV), lengths=t(lens.astype(np.int32)),
                           total_reward=t(D[P + "total_reward"].copy()), max_tile=t(D[P + "max_tile"].copy()),
                           final_boards=torch.zeros(W, n, dtype=torch.int64, device=DEV))


_exact: dict = {}


def _exact_grads(ci, u, case):
    """The update's pre-clip gradients in fp64 (oracle/agent_oracle.py, size-blind) at the reference's parameters."""
    if (ci, u) not in _exact:
        from oracle import agent_oracle as AO

        L = len(case["mlp"]["hidden_sizes"]) + 1
        crit = f"a{ci}_init_critic_0" in D
        ag = {k: v for k, v in case["agent"].items() if k != "model_seed"}
        ora = AO.OracleAgent(_before(ci, u, L, "actor"), _before(ci, u, L, "critic") if crit else None,
                             AO.AgentCfg(**ag, activation=case["mlp"]["activation"]), dtype=np.float64)
        ora.update_batch(_trajectories(ci, u, case))
        gW, gb = ora.captured["actor_grads"]
        out = {"actor": gW + gb}
        if crit:
            cW, cb = ora.captured["critic_grads"]
            out["critic"] = cW + cb
        _exact[(ci, u)] = out
    return _exact[(ci, u)]


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_rollout_matches_reference_run_episode(ci):
    case = CASES[ci]
    n_size, L = case["env"]["size"], len(case["mlp"]["hidden_sizes"]) + 1
    agent = _agent(case)
    assert agent.input_dim == n_size * n_size * (17 if case["env"]["obs_mode"] == "onehot" else 1)
    assert agent._net_spec() is None and agent._deep_spec() is None      # the fused kernels are not offered the net
    for u in range(case["updates"]):
        P = f"a{ci}_up{u}_"
        assert (D[P + "margin"] >= 1e-4).all()                            # the generator's seed condition
        _set(agent, _before(ci, u, L, "actor"))
        es, ps = [int(s) for s in D[P + "env_seeds"]], [int(s) for s in D[P + "policy_seeds"]]
        batch = agent.rollout_batch(es, ps, record_probs=True)
        path = agent.last_paths()["rollout"]
        assert "hipBLASLt forward" in path and "g2048_sample" in path and "g2048_sized_step" in path
        lens = D[P + "lengths"]
        np.testing.assert_array_equal(batch.lengths.cpu().numpy(), lens)
        W = (n_size * n_size + 15) // 16
        assert tuple(batch.boards.shape) == (W, int(lens.max()), len(lens)) and batch.T == int(lens.max())
        assert tuple(batch.final_boards.shape) == (W, len(lens)) and batch.rewards.dtype == torch.float64
        boards = _exps(batch.boards.cpu().numpy(), n_size)                # [T, n, N*N]
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
        # run_episode (one lane) returns the reference's trajectory dict
        tr = agent.run_episode(es[0], ps[0])
        assert tr["actions"] == [int(a) for a in D[P + "actions"][:int(lens[0])]]
        assert tr["rewards"] == [float(r) for r in D[P + "rewards"][:int(lens[0])]]
        o0 = tr["obs"][0]["board"] if case["env"].get("use_action_mask", True) else tr["obs"][0]
        assert o0.shape == ((n_size, n_size, 17) if case["env"]["obs_mode"] == "onehot" else (n_size, n_size))
        np.testing.assert_array_equal(o0, _obs(D[P + "boards"][0], case["env"])["board"])
        assert tr["states"][0].count("\n") == 2 * n_size and tr["max_tile"] == int(D[P + "max_tile"][0])
    # the Philox throughput mode runs the same path (same distribution, not the same stream)
    b2 = agent.rollout_batch(list(range(40)), list(range(100, 140)), rng="philox")
    ln = b2.lengths.cpu().numpy()
    assert (ln >= 1).all() and (ln <= case["env"]["max_steps"]).all() and bool(torch.isfinite(b2.total_reward).all())
    assert int(b2.max_tile.min()) >= 4


@pytest.mark.parametrize("path", ["device", "dropin"])
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_update_matches_reference_update_batch(ci, path):
    """The assertions of tests/test_gpu_ref_fixtures.py::test_update_matches_reference_update_batch on the sized
    cases: pre-clip gradients, norms, parameters after SGD / Adam (actor and critic), update after update."""
    case = CASES[ci]
    L = len(case["mlp"]["hidden_sizes"]) + 1
    agent = _agent(case)
    crit = f"a{ci}_init_critic_0" in D
    init = _params(ci, "init_actor", L)
    for a, b in zip(agent.params["W"] + agent.params["b"], init["W"] + init["b"]):
        np.testing.assert_array_equal(a.cpu().numpy(), b)
    if crit:
        cinit = _params(ci, "init_critic", L)
        for a, b in zip(agent.critic_params["W"] + agent.critic_params["b"], cinit["W"] + cinit["b"]):
            np.testing.assert_array_equal(a.cpu().numpy(), b)
    lr = case["agent"].get("learning_rate", 1e-3)
    lr_c = case["agent"].get("critic_learning_rate", 1e-3)
    adam = case["agent"].get("optimizer", "sgd") == "adam"
    b1, b2 = case["agent"].get("adam_beta1", 0.9), case["agent"].get("adam_beta2", 0.999)
    mx = case["agent"].get("max_grad_norm", 1.0)
    noisy_a = noisy_c = None
    for u in range(case["updates"]):
        P = f"a{ci}_up{u}_"
        if u:
            _set(agent, _before(ci, u, L, "actor"))
            if crit:
                _set(agent, _before(ci, u, L, "critic"), critic=True)
        before = [p.cpu().numpy().copy() for p in agent.params["W"] + agent.params["b"]]
        cbefore = [p.cpu().numpy().copy() for p in agent.critic_params["W"] + agent.critic_params["b"]] if crit \
            else None
        ast = RF.adam_state(agent) if adam else None
        cst = RF.adam_state(agent, critic=True) if adam and crit else None
        if path == "device":
            stats = agent.update_from_batch(_batch(ci, u, case))
        else:
            agent.update_batch(_trajectories(ci, u, case))
            stats = agent.last_stats
        paths = agent.last_paths()
        assert paths["actor_grad"] == "hipBLASLt backprop"
        if crit:
            assert paths["critic_grad"] == "hipBLASLt backprop"
        gref = [D[P + f"actor_grad_{j}"] for j in range(2 * L)]
        exact = lambda: _exact_grads(ci, u, case)  # noqa: E731
        for j, (g, r) in enumerate(zip(agent.last_grads["actor"], gref)):
            RF.assert_grad_parity(g.cpu().numpy(), r, lambda: exact()["actor"][j], (u, "actor", j))
        RF.assert_norm_parity(stats["actor_grad_norm"], float(D[P + "actor_norm"]), lambda: exact()["actor"],
                              (u, "actor norm"))
        ref, rb = _params(ci, f"up{u}_actor", L), _before(ci, u, L, "actor")
        after = [p.cpu().numpy() for p in agent.params["W"] + agent.params["b"]]
        noisy_a = assert_step_matches(after, before, ref["W"] + ref["b"], rb["W"] + rb["b"], gref, noisy_a, lr, adam)
        if adam:
            RF.assert_adam_step_exact(after, before, [g.cpu().numpy() for g in agent.last_grads["actor"]], ast, lr, 1.0,
                                      b1, b2, mx, (u, "actor"))
        if crit:
            cref = [D[P + f"critic_grad_{j}"] for j in range(2 * L)]
            for j, (g, r) in enumerate(zip(agent.last_grads["critic"], cref)):
                RF.assert_grad_parity(g.cpu().numpy(), r, lambda: exact()["critic"][j], (u, "critic", j))
            RF.assert_norm_parity(stats["critic_grad_norm"], float(D[P + "critic_norm"]), lambda: exact()["critic"],
                                  (u, "critic norm"))
            ref, rb = _params(ci, f"up{u}_critic", L), _before(ci, u, L, "critic")
            cafter = [p.cpu().numpy() for p in agent.critic_params["W"] + agent.critic_params["b"]]
            noisy_c = assert_step_matches(cafter, cbefore, ref["W"] + ref["b"], rb["W"] + rb["b"], cref, noisy_c,
                                          lr_c, adam)
            if adam:
                RF.assert_adam_step_exact(cafter, cbefore, [g.cpu().numpy() for g in agent.last_grads["critic"]], cst,
                                          lr_c, -1.0, b1, b2, mx, (u, "critic"))


def test_save_and_load_model(tmp_path):
    case = CASES[1]
    agent = _agent(case)
    f = str(tmp_path / "params.npz")
    agent.save_model(f)
    other = _agent(dict(case, agent=dict(case["agent"], model_seed=99)))
    other.load_model(f)
    for a, b in zip(agent.params["W"] + agent.params["b"], other.params["W"] + other.params["b"]):
        assert torch.equal(a, b)
    assert tuple(other.params["W"][0].shape)[0] == 25 * 17


def test_runner_matches_reference_training(tmp_path):
    """runner.training_loop at size 3 == the reference runner.py: every CSV row exactly, and the actor after the 2 SGD
    updates.  Final-actor bound: each update's gradient is within 1e-5 (normwise, of a clipped gradient of norm <= 1)
    of the reference's, so the parameters differ by at most 2 lr 1e-5, plus a few fp32 roundings of the parameter
    itself (rtol 1e-6)."""
    from rl2048_amd import runner as R

    conf = json.loads(str(D["r_conf"]))
    assert (D["r_margin"] >= 1e-4).all()
    R.reset_defaults()
    try:
        R.apply_config_overrides_from_dict(conf)
        agent, ec, mc, ac, tc = R.build_training_components(DEV)
        assert ec.size == 3 and agent.size == 3
        rows = R.training_loop(agent, ec, mc, ac, tc, tmp_path, "golden")
        assert [r["batch"] for r in rows] == list(D["r_batch"])
        for k in ("avg_reward", "max_reward", "min_reward"):
            np.testing.assert_array_equal([r[k] for r in rows], D["r_" + k], err_msg=k)
        assert [json.loads(r["max_tile_counts"]) for r in rows] == D["r_max_tile_counts"].tolist()
        header = (tmp_path / "training_stats.csv").read_text().splitlines()[0].split(",")
        assert header == json.loads(str(D["r_csv_header"]))
        assert "g2048_sized_step" in agent.last_paths()["rollout"]
        lr = conf["agent"]["learning_rate"]
        for j, p in enumerate(agent.params["W"] + agent.params["b"]):
            np.testing.assert_allclose(p.cpu().numpy(), D[f"r_final_actor_{j}"], rtol=1e-6, atol=2 * lr * 1e-5 + 1e-7,
                                       err_msg=f"tensor {j}")
    finally:
        R.reset_defaults()
