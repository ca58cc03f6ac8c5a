"""Generate the scripted-play fixtures from the REAL reference (build container only).

    python tests/golden/make_golden_scripted.py [--ref /root/reference]

Imports the reference the way make_golden_ref.py does (gym_shim, nothing written into its tree), plus its
tools/simple_action_gen.py, and writes tests/golden/scripted.npz (data only):

  masks       gen1_choice / gen2_choice [15]: action_gen_1 / action_gen_2 on the action masks 1..15 (bit a = action a)
  episodes    e{c}_*: ReinforceAgent.run_episode(env_seed, policy_seed, action_gen=action_gen_1 / _2)
              (src/reinforce_agent.py:195-252), 4 episodes per generator and case; per step the board before the step
              (uint8 exponents [rows, N*N], cell r*N+c), the action and the fp64 reward; per episode the generator (1 /
              2), seeds, length, total_reward and max_tile.  Cases ("ep_cases", JSON): 4 x 4 default config with
              max_steps None; 4 x 4 every-term config (tests/rollout_replay.CONFIGS["R-raw-mask"]) with max_steps None
              and 40; N = 3 and N = 5 under it; N = 8 with max_steps 48.  Cases with N >= 6 keep a finite max_steps
              (unbounded priority play on large boards runs for tens of thousands of steps).
  updates     u{ci}_*: update_batch on 4 teacher episodes (action_gen_2, 4 x 4, max_steps 60) in update.npz's per-case
              format (make_golden_ref.run_update_case records them; "update_cases" is the JSON list).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_ref as MR  # noqa: E402
from make_golden import seed_iter  # noqa: E402

# tests/rollout_replay.py: TERMS and CONFIGS["R-raw-mask"]
TERMS = dict(obs_log2_scale=0.3, base_reward_scale=1.0 / 3.0, empty_tile_reward=-0.07, merge_reward=0.3,
             bonus_scale=0.01, step_reward=-0.003, endgame_penalty=-7.3, invalid_action_penalty=-1.7)
R_RAW_MASK = dict(TERMS, reward_mode="log2", bonus_mode="raw", use_action_mask=True)

EP_CASES = [
    dict(name="4x4-default", size=4, env=dict(max_steps=None)),
    dict(name="4x4-terms", size=4, env=dict(R_RAW_MASK, max_steps=None)),
    dict(name="4x4-terms-40", size=4, env=dict(R_RAW_MASK, max_steps=40)),
    dict(name="3x3-terms", size=3, env=dict(R_RAW_MASK, max_steps=None)),
    dict(name="5x5-terms", size=5, env=dict(R_RAW_MASK, max_steps=None)),
    dict(name="8x8-terms-48", size=8, env=dict(R_RAW_MASK, max_steps=48)),
]
EPISODES = 4

MLP_16 = dict(hidden_sizes=[16, 16], activation="ReLU", init_distribution="HeNormal", last_init_normal=True)
ENV_T = dict(obs_mode="log2", obs_log2_scale=0.0625, reward_mode="log2", base_reward_scale=0.5, max_steps=60)
UPDATE_CASES = [
    dict(name="teacher-batch-sgd", env=ENV_T, mlp=MLP_16, n=4, updates=1,
         agent=dict(gamma=0.99, learning_rate=1e-2, baseline_mode="batch", optimizer="sgd", model_seed=300)),
    dict(name="teacher-critic-adam-huber", env=ENV_T, mlp=MLP_16, n=4, updates=1,
         agent=dict(gamma=0.99, learning_rate=1e-2, baseline_mode="batch", optimizer="adam", use_critic=True,
                    critic_loss_type="huber", huber_delta=0.5, critic_learning_rate=5e-3, model_seed=301)),
]


def exponents(board) -> np.ndarray:
    v = np.asarray(board, dtype=np.int64).reshape(-1)
    e = np.zeros(v.shape, dtype=np.uint8)
    nz = v > 0
    e[nz] = np.round(np.log2(v[nz])).astype(np.uint8)
    assert np.array_equal(np.where(nz, np.int64(1) << e.astype(np.int64), 0), v)
    return e


def gen_episodes(E, RA, M, gens, data):
    mlp = M.MLPConfig(hidden_sizes=[8], activation="ReLU")
    for c, case in enumerate(EP_CASES):
        env = E.Game2048Env(E.Game2048EnvConfig(size=case["size"], **case["env"]))
        agent = RA.ReinforceAgent(env, mlp, RA.ReinforceAgentConfig(model_seed=c))
        steplog = []
        orig_sel = agent.select_action

        def sel(obs, rng, action_fn=None, use_greedy=False, _o=orig_sel, _a=agent, _l=steplog):
            _l.append(exponents(_a.env.game.board))
            return _o(obs, rng, action_fn, use_greedy)

        agent.select_action = sel
        it_e, it_p = seed_iter(5000 + c), seed_iter(6000 + c)
        ep = {k: [] for k in ("gen", "env_seed", "policy_seed", "length", "total_reward", "max_tile")}
        acts, rews = [], []
        for g, fn in gens:
            for _ in range(EPISODES):
                es, ps = next(it_e), next(it_p)
                before = len(steplog)
                traj = agent.run_episode(es, ps, action_gen=fn)
                # the result must not depend on policy_seed: a second run under another policy seed
                again = agent.run_episode(es, ps ^ 0x5555, action_gen=fn)
                del steplog[before + len(traj["actions"]):]
                assert again["actions"] == traj["actions"] and again["rewards"] == traj["rewards"]
                assert len(steplog) - before == len(traj["actions"])
                ep["gen"].append(g)
                ep["env_seed"].append(es)
                ep["policy_seed"].append(ps)
                ep["length"].append(len(traj["actions"]))
                ep["total_reward"].append(traj["total_reward"])
                ep["max_tile"].append(traj["max_tile"])
                acts += traj["actions"]
                rews += traj["rewards"]
        P = f"e{c}_"
        dt = dict(gen=np.uint8, env_seed=np.uint64, policy_seed=np.uint64, length=np.int64, total_reward=np.float64,
                  max_tile=np.int64)
        for k, v in ep.items():
            data[P + k] = np.array(v, dtype=dt[k])
        data[P + "boards"] = np.stack(steplog).astype(np.uint8)
        data[P + "actions"] = np.array(acts, dtype=np.uint8)
        data[P + "rewards"] = np.array(rews, dtype=np.float64)
        print(f"  episodes {case['name']}: lengths {ep['length']}, max tiles {ep['max_tile']}")


def gen_updates(E, RA, M, gen2, data):
    def factory(env, mlp_cfg, agent_cfg):
        agent = RA.ReinforceAgent(env, mlp_cfg, agent_cfg)
        orig = agent.run_episode
        agent.run_episode = lambda es, ps: orig(es, ps, action_gen=gen2)   # teacher episodes
        return agent

    shim = types.SimpleNamespace(ReinforceAgent=factory, ReinforceAgentConfig=RA.ReinforceAgentConfig)
    for ci, case in enumerate(UPDATE_CASES):
        data.update(MR.run_update_case(E, shim, M, case, ci))
        print(f"  update {case['name']}: {int(data[f'u{ci}_up0_lengths'].sum())} steps")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    E, RA, M = MR.import_reference(args.ref)
    import tools.simple_action_gen as SG  # noqa: E402  (the reference's)

    data = {"ep_cases": np.array(json.dumps(EP_CASES)), "update_cases": np.array(json.dumps(UPDATE_CASES))}
    masks = [np.array([(m >> a) & 1 for a in range(4)], dtype=np.int8) for m in range(1, 16)]
    data["gen1_choice"] = np.array([SG.action_gen_1(None, m) for m in masks], dtype=np.uint8)
    data["gen2_choice"] = np.array([SG.action_gen_2(None, m) for m in masks], dtype=np.uint8)
    gen_episodes(E, RA, M, ((1, SG.action_gen_1), (2, SG.action_gen_2)), data)
    gen_updates(E, RA, M, SG.action_gen_2, data)
    out = os.path.join(HERE, "scripted.npz")
    np.savez_compressed(out, **data)
    print("wrote", out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < (1 << 20), "committed files stay below 1 MiB"


if __name__ == "__main__":
    main()
