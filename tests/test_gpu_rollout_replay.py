"""GPU: every episode of the four persistent rollout kernels replayed in the CPU oracles (tests/rollout_replay.py).

    rollout_kernel              g2048_rollout / g2048_rollout_eval               two hidden layers, log2 / raw
    deep_rollout_kernel<.., 32> g2048_deep_rollout / g2048_deep_eval             any depth, log2 / raw
    deep_rollout_kernel<.., 64> g2048_deep_rollout / g2048_deep_eval             one-hot
    sized_rollout_kernel<N>     g2048_sized_rollout / g2048_sized_eval           boards 2..8

Each keeps an episode's state (board, step count, score, max-tile exponent, fp64 running total, two PCG64 streams) in
registers, across a suspension in g2048_suspend, and refills a finished slot from a queue.  Here every row of every
episode of rollout_batch(record_probs=True) is held to the oracle (boards, fp64 reward bits, flags, the episode's end,
total, max tile, final board), the action to the recorded probabilities (numpy's Generator.choice restated, or the
first argmax) and the probabilities to an fp64 forward, under env configs in which every reward term is non-zero and
non-dyadic -- both bonus modes (the one term that depends on restored state), merge / step rewards, the endgame
penalty, and the action mask on and off (invalid moves, their penalty, the untouched env stream).

* test_terms_to_termination: 4 x 4, three families x four configs (+ one greedy run per family), n = 150 to the end;
  the deep families with a first capacity of 8 rows, so max_steps=None episodes are suspended and resumed repeatedly.
* test_invalid_run_to_truncation: greedy without a mask repeats its first invalid move until truncation.
* test_refilled_slots: n = 64 CUs + 3 * 64 + 37, the smallest shape at which slots take a second episode from the queue.
* test_sized_terms: N in {2, 3, 5, 6, 8}, 32 slots for 97 episodes, first capacity 8.
* test_score_only_under_the_same_terms: evaluate_batch (eval_step_budget = 8) equals the batches just replayed.

Left to other files on purpose: Philox streams (no persistent kernel takes them), tile saturation, and the forward at
large widths (tests/test_gpu_deep.py, tests/test_gpu_policy.py, tests/test_gpu_sized_policy.py): the nets here are
small, they only have to drive varied play.
"""
import numpy as np
import pytest
import torch

import rollout_replay as RR
from test_gpu_eval import DEEP_EVAL, FUSED_EVAL, SIZED_EVAL, _assert_same
from test_gpu_sized_rollout import NET_LOG2, NET_ONEHOT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

PATHS = {"two-layer": "g2048_rollout (one persistent launch)",
         "deep32": "g2048_deep_rollout (persistent launches, suspended episodes resumed)",
         "deep64": "g2048_deep_rollout (persistent launches, suspended episodes resumed)",
         "sized": "g2048_sized_rollout (persistent launches, suspended episodes resumed)"}
EVAL_PATHS = {"two-layer": FUSED_EVAL, "deep32": DEEP_EVAL, "deep64": DEEP_EVAL, "sized": SIZED_EVAL}
# small on purpose; two nets per family so that different tile instantiations (NT1 / NT2, depths) are reached
NETS = {"two-layer": [("log2", [40, 24], "ReLU"), ("raw", [33, 70], "Sigmoid")],
        "deep32": [("log2", [48], "ReLU"), ("raw", [24, 20, 12], "Sigmoid")],
        "deep64": [("onehot", [40, 24], "Sigmoid"), ("onehot", [64, 32, 16], "ReLU")]}
SIZED_NETS = [NET_LOG2, NET_ONEHOT, ("raw", [33], "Sigmoid")]
CONFIGS = list(RR.CONFIGS)
_done: dict = {}            # case id -> (agent, env seeds, policy seeds, batch, counts): computed once, left unchanged


def _agent(family, net, config, max_steps, size=4, seed=5):
    from rl2048_amd import Game2048EnvConfig
    from rl2048_amd.agent import ReinforceAgent, ReinforceAgentConfig
    from rl2048_amd.mlp import MLPConfig

    mode, hidden, act = net
    env = dict(RR.CONFIGS[config], obs_mode=mode, max_steps=max_steps)
    a = ReinforceAgent(Game2048EnvConfig(size=size, **env),
                       MLPConfig(hidden_sizes=hidden, activation=act, init_distribution="HeNormal"),
                       ReinforceAgentConfig(model_seed=seed), device=DEV)
    if mode == "raw":
        # raw obs reach 2^15: with O(1) first-layer weights the softmax saturates (tests/test_gpu_eval.py)
        a.params["W"][0].mul_(2.0 ** -12)
    a.deep_rollout_cap0 = 8
    if family == "sized":
        a.use_fused_sized_rollout, a.sized_rollout_cap0, a.sized_rollout_max_workgroups = True, 8, 1
    a.replay_env = env          # the oracle's config of this agent's env
    return a


def _replay(case, family, agent, n, base, greedy=False):
    """rollout_batch on n seeded episodes through the family's persistent kernel, then every row of it through the
    replay, the choice check and the probability check.  Cached under `case`."""
    if case not in _done:
        es = np.arange(base, base + n, dtype=np.int64)
        ps = es + 10 ** 9
        batch = agent.rollout_batch(es, ps, use_greedy=greedy, record_probs=True)
        assert agent.last_paths()["rollout"] == PATHS[family], agent.last_paths()
        assert (agent.env_config.obs_mode == "onehot") == (family == "deep64") or family == "sized"
        size = agent.env_config.size
        if family == "sized":
            c = RR.replay_sized(batch, size, agent.replay_env, es)
        else:
            c = RR.replay_4x4(batch, agent.replay_env, es)
        assert c["rows"] == int(batch.lengths.sum())
        assert RR.check_choices(batch.probs, batch.actions, batch.lengths, ps, greedy, c["masks"]) == c["rows"]
        c["ratio"] = RR.check_probs(agent, batch, c["masks"], label=case)
        print(case, {k: v for k, v in c.items() if k != "masks"}, "T", batch.T, "median length",
              int(batch.lengths.median()), flush=True)
        _done[case] = (agent, es, ps, batch, c)
    return _done[case]


# ------------------------------------------------------------------------------------------- a. terms to termination
TERM_CASES = [(f, k, False) for f in NETS for k in range(4)] + [(f, 3, True) for f in NETS]


def _term_id(f, k, greedy):
    return f"{f}-{CONFIGS[k]}" + ("-greedy" if greedy else "")


def _term_case(f, k, greedy):
    config = CONFIGS[k]
    mask_on = RR.CONFIGS[config]["use_action_mask"]
    max_steps = 200 if (f == "two-layer" or not mask_on) else None
    net = NETS[f][(k + greedy) % 2]                      # the greedy run takes the net config 3 does not
    case = _term_id(f, k, greedy)
    if case in _done:
        return _done[case] + (max_steps,)
    a = _agent(f, net, config, max_steps)
    return _replay(case, f, a, 150, 100_000 + 1000 * (4 * list(NETS).index(f) + k) + 500 * greedy, greedy) + (max_steps,)


@pytest.mark.parametrize("f,k,greedy", TERM_CASES, ids=[_term_id(*c) for c in TERM_CASES])
def test_terms_to_termination(f, k, greedy):
    """n = 150 (ragged for both slot counts).  Two-layer: max_steps = 200, both endings.  Deep families: max_steps None
    with the mask on (every episode is suspended at 8, 16, 32, ... rows and resumed) and 200 with it off."""
    a, es, ps, b, c, max_steps = _term_case(f, k, greedy)
    assert c["terminated"] > 0, c["terminated"]          # the endgame penalty was paid
    assert c["merges"] > 0 and c["bonus"] > 0
    assert c["terminated"] + c["truncated"] == 150
    if not a.env_config.use_action_mask:
        assert c["invalid"] > 0
    else:
        assert c["invalid"] == 0
    if max_steps is not None:
        assert c["truncated"] > 0
    else:
        assert c["truncated"] == 0
    if f != "two-layer":
        assert b.T > 8 and int(b.lengths.median()) > 16


# ------------------------------------------------------------------------------------ b. invalid run to truncation
@pytest.mark.parametrize("f", ["deep32", "deep64"])
def test_invalid_run_to_truncation(f):
    """No mask, greedy, max_steps = 40, n = 70: the policy repeats its first invalid move until truncation.  In those
    rows the board does not change and the reward is exactly the penalty; the replay's checks of the following rows
    and of the final board prove that the env stream was not advanced (the oracle's next spawn would differ)."""
    from rl2048_amd import _lib as L

    config = "R-log2-nomask"
    a = _agent(f, NETS[f][0], config, 40)
    _, es, ps, b, c = _replay(f"invalid-run-{f}", f, a, 70, 200_000, greedy=True)
    assert c["invalid"] > 0 and c["truncated"] > 0
    flags, lens = b.flags.cpu().numpy(), b.lengths.cpu().numpy()
    boards, rewards, final = b.boards.cpu().numpy(), b.rewards.cpu().numpy(), b.final_boards.cpu().numpy()
    longest = 0
    for i in range(70):
        inv = (flags[:lens[i], i] & L.F_INVALID) != 0
        run = 0
        while run < lens[i] and inv[lens[i] - 1 - run]:
            run += 1
        longest = max(longest, run)
        if run >= 5:
            rows = np.arange(lens[i] - run, lens[i])
            assert lens[i] == 40 and (flags[rows[-1], i] & L.F_TRUNCATED) != 0
            assert (boards[rows, i] == boards[rows[0], i]).all() and final[i] == boards[rows[0], i]
            assert (rewards[rows, i] == RR.TERMS["invalid_action_penalty"]).all()
            assert ((flags[rows, i] & L.F_CHANGED) == 0).all()
            assert len(np.unique(b.actions.cpu().numpy()[rows, i])) == 1
    assert longest >= 5, longest


# ------------------------------------------------------------------------------------------------ c. refilled slots
@pytest.mark.parametrize("config", ["R-raw-mask", "R-log2-nomask"])
@pytest.mark.parametrize("f", list(NETS))
def test_refilled_slots(f, config):
    """n = 64 CUs + 3 * 64 + 37: the persistent grid is capped (64 slots per CU) and slots take a second episode from
    the queue -- the only shape at which a stale max-tile exponent, step count, score or total after start() can
    show.  max_steps = 24: every episode is replayed, 24 EnvBatch steps."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 64 * cus + 3 * 64 + 37
    k = CONFIGS.index(config)
    a = _agent(f, NETS[f][k % 2], config, 24)
    _, es, ps, b, c = _replay(f"refill-{f}-{config}", f, a, n, 300_000 + 100_000 * k)
    assert c["terminated"] + c["truncated"] == n and c["truncated"] > 0
    assert b.T == 24
    assert c["bonus"] >= n, c["bonus"]
    assert c["merges"] > 0 and (c["invalid"] > 0) == (not a.env_config.use_action_mask)
    _done.pop(f"refill-{f}-{config}")               # the largest batches of the file: not kept


# --------------------------------------------------------------------------------------------------- d. sized terms
PAIRS = (("R-raw-mask", "R-log2-nomask"), ("S-raw-nomask", "L-log2-mask"))   # each: both bonus modes, the mask off once
SIZED_CASES = [(size, config, SIZED_NETS[(i + j) % 3])
               for i, size in enumerate((2, 3, 5, 6, 8)) for j, config in enumerate(PAIRS[i % 2])]


def _sized_id(size, config, net):
    return f"N{size}-{config}-{net[0]}"


def _sized_case(size, config, net):
    case = _sized_id(size, config, net)
    if case in _done:
        return _done[case]
    a = _agent("sized", net, config, 40, size=size, seed=size)
    assert a._sized_spec() is not None
    return _replay(case, "sized", a, 97, 400_000 + 1000 * size + 100 * CONFIGS.index(config))


@pytest.mark.parametrize("size,config,net", SIZED_CASES, ids=[_sized_id(*c) for c in SIZED_CASES])
def test_sized_terms(size, config, net):
    """n = 97, max_steps = 40, one workgroup (32 slots: every slot refills twice), first capacity 8 (episodes are
    suspended as the buffer doubles).  W = 1, 1, 2, 3, 4 words."""
    a, es, ps, b, c = _sized_case(size, config, net)
    assert c["terminated"] + c["truncated"] == 97
    if size <= 3:
        assert c["terminated"] > 0
    else:
        assert c["truncated"] > 0 and b.T == 40
    assert c["bonus"] > 0 and c["merges"] > 0
    assert (c["invalid"] > 0) == (not a.env_config.use_action_mask)
    assert b.T > 8


# --------------------------------------------------------------------------------------------------- e. score only
EVAL_CASES = [("two-layer", 1), ("deep32", 2), ("deep64", 0), ("deep64", 1), ("sized", 3), ("sized", 6)]


@pytest.mark.parametrize("f,k", EVAL_CASES, ids=[f"{f}-{k}" for f, k in EVAL_CASES])
def test_score_only_under_the_same_terms(f, k):
    """evaluate_batch on the seeds of a case above, suspended every 8 steps, equals the batch just replayed: lengths,
    totals (fp64 bits), max tile, final boards.  With a finite max_steps the trajectory kernel was not suspended
    through the agent but the score-only one is: truncation then comes from a restored step count, and the bonus
    depends on a restored max-tile exponent."""
    if f == "sized":
        a, es, ps, b, c = _sized_case(*SIZED_CASES[k])
    else:
        a, es, ps, b, c, _ = _term_case(f, k, False)
    assert int(b.lengths.max()) > 8                 # the score-only kernel suspends these episodes at least once
    a.eval_step_budget = 8
    try:
        ev = a.evaluate_batch(es, ps, use_greedy=False)
    finally:
        del a.eval_step_budget
    assert EVAL_PATHS[f] in a.last_paths()["eval"], a.last_paths()
    _assert_same(ev, b)
