"""Generate the board-size fixtures (sizes 2..8) from the REAL reference (build container only).

    python tests/golden/make_golden_sized.py [--ref /root/reference]

Imports the reference's own modules by package path from ``--ref`` with ``sys.dont_write_bytecode`` set, through
tests/golden/gym_shim/ like make_golden_ref.py, runs them unchanged and records inputs / outputs.  Writes
tests/golden/sized.npz and tests/golden/sized_agent.npz (data only).  Boards are stored as uint8 exponents [..., N*N] (log2 of the tile, 0 = empty,
row-major); merged lists as uint8 exponents padded with zeros to N*(N//2).

  lines     n{N}_line_in / _out / _merged: Game2048._row_move_left (src/game2048.py:120-137) on every line over
            exponents {0,1,2} (3**N lines) and crafted lines holding 14 and 15 (the reference's output may hold 16)
  crafted   n{N}_craft_board / _mask / _done: get_action_mask and _is_done on hand-made boards
  env       n{N}_c{c}_*: Game2048Env.reset / step under ENV_CFGS[c] for c in ENV_SEL, 4 episodes each
  sym       n{N}_s{k}_*: Game2048Env.get_symmetries at N = 3, 5 on log2-dict and one-hot-dict observations
  agent     a{ci}_*: ReinforceAgent.run_episode + update_batch (src/reinforce_agent.py:195-620) at sizes 3 and 5, recorded
            as update.npz records them (trajectories, probabilities, pre-clip gradients, norms, post-update parameters)
  runner    r_*: the reference runner.py training loop at size 3 (CSV rows + final actor), as runner.npz records it

Seed selection for the agent and runner episodes is a condition, not a measurement: the device forward agrees with
the reference's probabilities to 2e-6 (the bound of tests/test_gpu_ref_fixtures.py), four of which accumulate to a cdf
error of about 8e-6, so only (env_seed, policy_seed) pairs are kept for which every sampling draw lies at least
MARGIN = 1e-4 from every cdf boundary of Generator.choice (asserted for every stored step): the GPU tests then replay
the same actions without skipping anything.
"""
from __future__ import annotations

import argparse
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import seed_iter  # noqa: E402
from make_golden_ref import ENV_CFGS, import_reference  # noqa: E402

SIZES = [2, 3, 5, 6, 7, 8]
ENV_SEL = [1, 2, 3, 4]   # log2 / sum + every bonus / one-hot without mask / raw without mask and max_steps None


def exps(board) -> np.ndarray:
    b = np.asarray(board, dtype=np.int64).reshape(-1)
    e = np.zeros(b.shape, dtype=np.uint8)
    nz = b > 0
    e[nz] = np.log2(b[nz]).astype(np.uint8)
    assert np.array_equal(np.where(e > 0, np.int64(1) << e.astype(np.int64), 0), b)
    return e


def vals(e) -> np.ndarray:
    e = np.asarray(e, dtype=np.int64)
    return np.where(e > 0, np.int64(1) << e, 0).astype(np.int64)


def pad_merged(merged, size) -> np.ndarray:
    out = np.zeros(size * (size // 2), dtype=np.uint8)
    out[:len(merged)] = [int(v).bit_length() - 1 for v in merged]
    return out


def mask_bits(m) -> int:
    return int(sum(int(b) << i for i, b in enumerate(m)))


def gen_lines(G, data):
    for n in range(2, 9):
        g = G(size=n)
        lines = [list(t) for t in itertools.product((0, 1, 2), repeat=n)]
        hi = [[15] * n, [14] * n, [15, 15] + [0] * (n - 2), [0] * (n - 2) + [15, 15], [14, 14, 15][:n] + [0] * max(n - 3, 0),
              ([15, 0, 15, 14, 14, 13, 13, 15] * 2)[:n], ([14, 15, 15, 14, 0, 15, 0, 15])[:n],
              ([1, 15, 15, 15, 2, 2, 14, 14])[:n]]
        lines += hi
        outs, mer = [], []
        for ln in lines:
            g._new_merged = []
            o = g._row_move_left(vals(ln))
            outs.append(exps(o))
            m = np.zeros(max(n // 2, 1), dtype=np.uint8)
            m[:len(g._new_merged)] = [int(v).bit_length() - 1 for v in g._new_merged]
            mer.append(m)
        data[f"n{n}_line_in"] = np.array(lines, dtype=np.uint8)
        data[f"n{n}_line_out"] = np.array(outs, dtype=np.uint8)
        data[f"n{n}_line_merged"] = np.array(mer, dtype=np.uint8)


def crafted_boards(n: int, rng) -> list[np.ndarray]:
    r, c = np.indices((n, n))
    checker = 1 + ((r + c) % 2)                       # full, no equal neighbours: done
    out = [checker]
    b = checker.copy()                                # only equal pair in the last row
    b[n - 1, n - 1] = b[n - 1, n - 2]
    if n > 1 and n - 2 >= 0 and b[n - 2, n - 1] == b[n - 1, n - 1]:
        b[n - 2, n - 1] = 3
    out.append(b)
    b = checker.copy()                                # only equal pair in the last column
    b[n - 1, n - 1] = b[n - 2, n - 1]
    if b[n - 1, n - 2] == b[n - 1, n - 1]:
        b[n - 1, n - 2] = 3
    out.append(b)
    b = checker.copy()                                # single empty cell: the last cell of the last word
    b[n - 1, n - 1] = 0
    out.append(b)
    b = checker.copy()                                # single empty cell: the first cell
    b[0, 0] = 0
    out.append(b)
    out.append(np.tile(1 + np.arange(n)[:, None], (1, n)))       # all-equal rows
    out.append(np.tile(1 + np.arange(n)[None, :], (n, 1)))       # all-equal columns
    out.append(np.zeros((n, n), dtype=np.int64))
    e = np.zeros((n, n), dtype=np.int64)                          # one tile in each corner in turn
    for (i, j) in ((0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1)):
        x = e.copy()
        x[i, j] = 5
        out.append(x)
    for _ in range(40):                                           # random fills
        x = rng.integers(1, 6, size=(n, n))
        x[rng.random((n, n)) < rng.choice([0.0, 0.1, 0.5])] = 0
        out.append(x)
    return [np.asarray(x, dtype=np.int64) for x in out]


def gen_crafted(G, data):
    rng = np.random.default_rng(77)
    for n in SIZES:
        g = G(size=n)
        boards, masks, dones = [], [], []
        for e in crafted_boards(n, rng):
            g.board = vals(e)
            boards.append(e.reshape(-1))
            masks.append(mask_bits(g.get_action_mask()))
            dones.append(bool(g._is_done()))
        assert dones[0] and not dones[1] and not dones[2] and masks[1] and masks[2], (n, dones[:3], masks[:3])
        data[f"n{n}_craft_board"] = np.array(boards, dtype=np.uint8)
        data[f"n{n}_craft_mask"] = np.array(masks, dtype=np.uint8)
        data[f"n{n}_craft_done"] = np.array(dones, dtype=np.bool_)


def obs_flat(obs):
    board = obs["board"] if isinstance(obs, dict) else obs
    return np.asarray(board, dtype=np.float32).reshape(-1)


def gen_env(E, data):
    rng = np.random.default_rng(4096)
    it = seed_iter(23)
    data["env_cfgs"] = np.array(json.dumps({str(c): ENV_CFGS[c] for c in ENV_SEL}))
    for n in SIZES:
        for c in ENV_SEL:
            cfg = E.Game2048EnvConfig(size=n, **ENV_CFGS[c])
            env = E.Game2048Env(cfg)
            cap = 60 if n >= 5 else 100000
            keys = ("action", "board", "reward", "terminated", "truncated", "invalid", "max_tile_seen", "score",
                    "step_index", "mask", "obs", "merged")
            st = {k: [] for k in keys}
            ep = {k: [] for k in ("seed", "start", "len", "reset_board", "reset_obs", "reset_mask")}
            for e in range(4):
                seed = next(it)
                obs, info = env.reset(seed=seed)
                ep["seed"].append(seed)
                ep["start"].append(len(st["action"]))
                ep["reset_board"].append(exps(env.game.board))
                ep["reset_obs"].append(obs_flat(obs))
                ep["reset_mask"].append(mask_bits(env.game.get_action_mask()))
                t = 0
                while t < cap:
                    m = env.game.get_action_mask()
                    valid = [i for i, v in enumerate(m) if v]
                    a = int(rng.integers(4)) if (e < 2 or not valid) else int(valid[int(rng.integers(len(valid)))])
                    obs, r, term, trunc, info = env.step(a)
                    assert isinstance(r, float)
                    st["action"].append(a)
                    st["board"].append(exps(env.game.board))
                    st["reward"].append(r)
                    st["terminated"].append(term)
                    st["truncated"].append(trunc)
                    st["invalid"].append(bool(info["invalid_action"]))
                    st["max_tile_seen"].append(env.max_tile_seen)
                    st["score"].append(info["score"])
                    st["step_index"].append(info["step_index"])
                    st["mask"].append(mask_bits(env.game.get_action_mask()))
                    st["obs"].append(obs_flat(obs))
                    st["merged"].append(pad_merged(info["merged"], n))
                    t += 1
                    if term or trunc:
                        break
                ep["len"].append(t)
            p = f"n{n}_c{c}_"
            data[p + "ep_seed"] = np.array(ep["seed"], dtype=np.uint64)
            data[p + "ep_start"] = np.array(ep["start"], dtype=np.int64)
            data[p + "ep_len"] = np.array(ep["len"], dtype=np.int64)
            data[p + "reset_board"] = np.array(ep["reset_board"], dtype=np.uint8)
            data[p + "reset_obs"] = np.array(ep["reset_obs"], dtype=np.float32)
            data[p + "reset_mask"] = np.array(ep["reset_mask"], dtype=np.uint8)
            dt = dict(action=np.uint8, board=np.uint8, reward=np.float64, terminated=np.bool_, truncated=np.bool_,
                      invalid=np.bool_, max_tile_seen=np.int64, score=np.int64, step_index=np.int64, mask=np.uint8,
                      obs=np.float32, merged=np.uint8)
            for k, v in st.items():
                data[p + k] = np.array(v, dtype=dt[k])
            print(f"  size {n} cfg {c}: lens {ep['len']}, {int(np.sum(st['terminated']))} terminated, "
                  f"{int(np.sum(st['truncated']))} truncated, {int(np.sum(st['invalid']))} invalid")


def gen_sym(E, data):
    rng = np.random.default_rng(9)
    for n in (3, 5):
        for k, mode in enumerate(("log2", "onehot")):
            env = E.Game2048Env(E.Game2048EnvConfig(size=n, obs_mode=mode, obs_log2_scale=0.25))
            env.reset(seed=0)
            e_in, a_in, b_out, m_out, a_out = [], [], [], [], []
            for i in range(12):
                e = rng.integers(0, 12, size=(n, n))
                env.game.board = vals(e)
                obs = env._get_obs()
                for a in range(4):
                    syms = E.Game2048Env.get_symmetries(obs, a)
                    assert len(syms) == 8
                    e_in.append(e.reshape(-1))
                    a_in.append(a)
                    b_out.append([obs_flat(s[0]) for s in syms])
                    m_out.append([s[0]["action_mask"] for s in syms])
                    a_out.append([s[1] for s in syms])
            p = f"n{n}_s{k}_"
            data[p + "board_in"] = np.array(e_in, dtype=np.uint8)
            data[p + "action_in"] = np.array(a_in, dtype=np.uint8)
            data[p + "obs_out"] = np.array(b_out, dtype=np.float32)
            data[p + "mask_out"] = np.array(m_out, dtype=np.int8)
            data[p + "action_out"] = np.array(a_out, dtype=np.uint8)
    data["sym_kinds"] = np.array(json.dumps([["log2", 0.25], ["onehot", 0.25]]))


MARGIN = 1e-4

AGENT_CASES = [
    dict(name="size3-reinforce-sgd-log2",
         env=dict(size=3, obs_mode="log2", obs_log2_scale=0.25, reward_mode="log2", base_reward_scale=0.5, max_steps=40),
         mlp=dict(hidden_sizes=[32], activation="ReLU", init_distribution="HeNormal", last_init_normal=True),
         agent=dict(gamma=0.99, learning_rate=1e-2, baseline_mode="batch", optimizer="sgd", model_seed=3),
         n=6, updates=2),
    dict(name="size5-critic-adam-onehot-aug",
         env=dict(size=5, obs_mode="onehot", reward_mode="sum", base_reward_scale=0.1, empty_tile_reward=0.01,
                  max_steps=30),
         mlp=dict(hidden_sizes=[64, 32], activation="ReLU", init_distribution="HeNormal", last_init_normal=True),
         agent=dict(gamma=0.99, learning_rate=1e-2, baseline_mode="batch", optimizer="adam", use_critic=True,
                    critic_learning_rate=5e-3, augmentation=True, model_seed=5),
         n=6, updates=2),
]


def _params_flat(p):
    return [np.array(a, dtype=np.float32, copy=True) for a in list(p["W"]) + list(p["b"])]


def draw_margin(rng, probs) -> float:
    """Distance of the uniform draw Generator.choice(4, p=probs) is about to take from the nearest cdf boundary
    (the generator is left where it was)."""
    st = rng.bit_generator.state
    u = rng.random()
    rng.bit_generator.state = st
    cdf = np.cumsum(np.asarray(probs, dtype=np.float64))
    cdf /= cdf[-1]
    return float(np.min(np.abs(cdf[:-1] - u)))


def watch_agent(agent, steplog):
    """Record (board exponents, action, probs, draw margin) of every select_action call."""
    orig = agent.select_action

    def sel(obs, rng, action_fn=None, use_greedy=False):
        b = exps(agent.env.game.board)
        # the probabilities first: the reference computes them inside select_action, so it is called once with the
        # generator put back afterwards, the margin of the coming draw is taken, then the real call draws
        st = rng.bit_generator.state
        _, probs, _, _ = orig(obs, rng, action_fn, use_greedy)
        rng.bit_generator.state = st
        margin = draw_margin(rng, probs)
        a, probs2, acts, pres = orig(obs, rng, action_fn, use_greedy)
        assert np.array_equal(probs, probs2)
        steplog.append((b, a, np.asarray(probs, dtype=np.float32).copy(), margin))
        return a, probs2, acts, pres

    agent.select_action = sel


def run_agent_case(E, RA, M, case, ci):
    env = E.Game2048Env(E.Game2048EnvConfig(**case["env"]))
    agent = RA.ReinforceAgent(env, M.MLPConfig(**case["mlp"]), RA.ReinforceAgentConfig(**case["agent"]))
    out, P = {}, f"a{ci}_"
    for j, a in enumerate(_params_flat(agent.params)):
        out[P + f"init_actor_{j}"] = a
    if agent.critic_params is not None:
        for j, a in enumerate(_params_flat(agent.critic_params)):
            out[P + f"init_critic_{j}"] = a
    steplog: list = []
    watch_agent(agent, steplog)
    cap: dict = {}
    orig_clip = agent.clip_grads_global_norm

    def clip(gW, gb):
        cap.setdefault("grads", []).append([np.array(g, dtype=np.float32) for g in list(gW) + list(gb)])
        nrm = orig_clip(gW, gb)
        cap.setdefault("norms", []).append(float(nrm))
        return nrm

    agent.clip_grads_global_norm = clip
    it_e, it_p = seed_iter(3000 + ci), seed_iter(4000 + ci)
    for u in range(case["updates"]):
        kept, tried = [], 0
        while len(kept) < case["n"]:
            e_s, p_s = next(it_e), next(it_p)
            tried += 1
            steplog.clear()
            tr = agent.run_episode(e_s, p_s)
            if min(s[3] for s in steplog) >= MARGIN:
                kept.append((e_s, p_s, tr, list(steplog)))
        trajs = [k[2] for k in kept]
        steps = [s for k in kept for s in k[3]]
        assert all(s[3] >= MARGIN for s in steps)
        lens = np.array([len(t["actions"]) for t in trajs], dtype=np.int64)
        assert len(steps) == lens.sum()
        Q = P + f"up{u}_"
        out[Q + "env_seeds"] = np.array([k[0] for k in kept], dtype=np.uint64)
        out[Q + "policy_seeds"] = np.array([k[1] for k in kept], dtype=np.uint64)
        out[Q + "lengths"] = lens
        out[Q + "boards"] = np.array([s[0] for s in steps], dtype=np.uint8)
        out[Q + "actions"] = np.array([s[1] for s in steps], dtype=np.uint8)
        out[Q + "probs"] = np.array([s[2] for s in steps], dtype=np.float32)
        out[Q + "margin"] = np.array([s[3] for s in steps], dtype=np.float64)
        out[Q + "rewards"] = np.concatenate([np.array(t["rewards"], dtype=np.float64) for t in trajs])
        out[Q + "total_reward"] = np.array([t["total_reward"] for t in trajs], dtype=np.float64)
        out[Q + "max_tile"] = np.array([t["max_tile"] for t in trajs], dtype=np.int64)
        cap.clear()
        agent.update_batch(trajs)
        out[Q + "actor_norm"] = np.array(cap["norms"][0], dtype=np.float64)
        for j, g in enumerate(cap["grads"][0]):
            out[Q + f"actor_grad_{j}"] = g
        for j, a in enumerate(_params_flat(agent.params)):
            out[Q + f"actor_{j}"] = a
        if agent.critic_params is not None:
            out[Q + "critic_norm"] = np.array(cap["norms"][1], dtype=np.float64)
            for j, g in enumerate(cap["grads"][1]):
                out[Q + f"critic_grad_{j}"] = g
            for j, a in enumerate(_params_flat(agent.critic_params)):
                out[Q + f"critic_{j}"] = a
        print(f"  agent case {ci} update {u}: {int(lens.sum())} steps, kept {len(kept)} of {tried} seed pairs, "
              f"min margin {min(s[3] for s in steps):.2e}")
    return out


def gen_agent(E, RA, M, data):
    data["agent_cases"] = np.array(json.dumps(AGENT_CASES))
    for ci, case in enumerate(AGENT_CASES):
        data.update(run_agent_case(E, RA, M, case, ci))


RUNNER_CONF = {
    "env": dict(size=3, obs_mode="log2", obs_log2_scale=0.25, reward_mode="log2", base_reward_scale=0.5, max_steps=40),
    "mlp": dict(hidden_sizes=[32, 16], activation="ReLU", init_distribution="HeNormal", last_init_normal=True),
    "agent": dict(gamma=0.99, learning_rate=1e-2, baseline_mode="batch", model_seed=0, optimizer="sgd"),
    "train": dict(batch_size=4, num_batches=2, env_base_seed=3, policy_base_seed=7),
}


def gen_runner(data):
    import csv
    import logging
    import tempfile
    from pathlib import Path

    import runner as R  # noqa: E402  (the reference runner.py, on sys.path via import_reference)

    for attempt in range(200):
        conf = json.loads(json.dumps(RUNNER_CONF))
        conf["train"]["env_base_seed"] += attempt
        conf["train"]["policy_base_seed"] += 2 * attempt
        R.apply_config_overrides_from_dict(json.loads(json.dumps(conf)))
        env, agent, env_config, mlp_config, agent_config, train_cfg = R.build_training_components()
        steplog: list = []
        watch_agent(agent, steplog)
        with tempfile.TemporaryDirectory() as td:
            R.training_loop(env, agent, env_config, mlp_config, agent_config, train_cfg, Path(td), "golden")
            with open(os.path.join(td, "training_stats.csv"), newline="") as f:
                rows = list(csv.DictReader(f))
            root = logging.getLogger()
            for h in list(root.handlers):
                if isinstance(h, logging.FileHandler):
                    root.removeHandler(h)
                    h.close()
        if min(s[3] for s in steplog) >= MARGIN:
            break
    else:
        raise SystemExit("no runner base seeds with every draw clear of the cdf boundaries")
    assert all(s[3] >= MARGIN for s in steplog)
    print(f"  runner: base seeds attempt {attempt}, {len(steplog)} steps, min margin {min(s[3] for s in steplog):.2e}")
    data["r_conf"] = np.array(json.dumps(conf))
    data["r_batch"] = np.array([int(x["batch"]) for x in rows], dtype=np.int64)
    for k in ("avg_reward", "max_reward", "min_reward"):
        data["r_" + k] = np.array([float(x[k]) for x in rows], dtype=np.float64)
    data["r_max_tile_counts"] = np.array([json.loads(x["max_tile_counts"]) for x in rows], dtype=np.int64)
    data["r_csv_header"] = np.array(json.dumps(list(rows[0].keys())))
    data["r_margin"] = np.array([s[3] for s in steplog], dtype=np.float64)
    for j, a in enumerate(_params_flat(agent.params)):
        data[f"r_final_actor_{j}"] = a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    E, RA, M = import_reference(args.ref)
    from src.game2048 import Game2048 as G
    data = {"sizes": np.array(SIZES), "env_sel": np.array(ENV_SEL)}
    gen_lines(G, data)
    gen_crafted(G, data)
    gen_env(E, data)
    gen_sym(E, data)
    # the agent / runner records (mostly fp32 parameters and gradients) go to a file of their own: each stays below
    # the repository's 1 MiB limit for a committed file
    agent_data: dict = {}
    gen_agent(E, RA, M, agent_data)
    gen_runner(agent_data)
    for name, d in (("sized.npz", data), ("sized_agent.npz", agent_data)):
        out = os.path.join(HERE, name)
        np.savez_compressed(out, **d)
        print("wrote", out, os.path.getsize(out), "bytes")
        assert os.path.getsize(out) < (1 << 20), "committed files stay below 1 MiB"


if __name__ == "__main__":
    main()
