"""GPU: score-only evaluation rollouts -- ReinforceAgent.evaluate_batch over g2048_rollout_eval, g2048_deep_eval and
g2048_sized_eval (the persistent rollout kernels instantiated without their trajectory row), and the runner's
evaluation_loop(score_only=True).

The yardstick is rollout_batch of the same agent on the same seeds: the score-only kernels are the trajectory kernels'
code minus the row stores, so every comparison is exact -- torch.equal on the int fields, and on the fp64 totals through
.view(torch.int64).  The trajectory kernels are pinned to the reference by the fixture tests, and their suspend / resume
to stepwise play by test_deep_rollout_suspend_resume_equals_stepwise, so equality with them is equality with the
reference.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

DEEP_EVAL = "g2048_deep_eval"
SIZED_EVAL = "g2048_sized_eval"
FUSED_EVAL = "g2048_rollout_eval"
FIELDS = ("lengths", "total_reward", "max_tile", "final_boards")


def _agent(size, mode, hidden, act, seed=5, **env):
    from rl2048_amd import Game2048EnvConfig
    from rl2048_amd.agent import ReinforceAgent, ReinforceAgentConfig
    from rl2048_amd.mlp import MLPConfig

    kw = dict(obs_log2_scale=0.125, max_steps=None, use_action_mask=True, reward_mode="log2", empty_tile_reward=0.05)
    cfg = Game2048EnvConfig(size=size, obs_mode=mode, **dict(kw, **env))
    a = ReinforceAgent(cfg, MLPConfig(hidden_sizes=hidden, activation=act, init_distribution="HeNormal"),
                       ReinforceAgentConfig(model_seed=seed), device=DEV)
    if mode == "raw":
        # raw obs reach 2^15: with O(1) first-layer weights the softmax saturates (tests/test_gpu_sized_grad.py)
        a.params["W"][0].mul_(2.0 ** -12)
    return a


def _seeds(n, base):
    es = np.arange(base, base + n, dtype=np.int64)
    return es, es + 10 ** 9


def _assert_same(ev, tb):
    """The four EvalBatch fields against the TrajectoryBatch fields of those names: dtype, shape and every bit."""
    assert ev.n == tb.n
    for name in FIELDS:
        x, y = getattr(ev, name), getattr(tb, name)
        assert x.dtype == y.dtype and tuple(x.shape) == tuple(y.shape), name
        if x.dtype == torch.float64:
            x, y = x.view(torch.int64), y.view(torch.int64)
        assert torch.equal(x, y), name


# ----------------------------------------------------------------------------------------------- 1. deep family
DEEP_NETS = {"onehot64": ("onehot", [40, 24], "Sigmoid"), "log2_32": ("log2", [48], "ReLU")}
_deep_ref: dict = {}


def _deep_case(net, greedy):
    """(agent, seeds, rollout_batch's batch) of one deep-family case: computed once, shared, left unchanged."""
    key = (net, greedy)
    if key not in _deep_ref:
        a = _agent(4, *DEEP_NETS[net])
        es, ps = _seeds(150, 7000 + 1000 * len(_deep_ref))     # three 64-slot workgroups, the last one ragged
        tb = a.rollout_batch(es, ps, use_greedy=greedy)
        assert a.last_paths()["rollout"].startswith("g2048_deep_rollout")
        _deep_ref[key] = (a, es, ps, tb)
    return _deep_ref[key]


@pytest.mark.parametrize("greedy", [False, True], ids=["sampled", "greedy"])
@pytest.mark.parametrize("net", list(DEEP_NETS))
def test_deep_family_equals_its_trajectory_kernel(net, greedy):
    """4 x 4, max_steps None, n = 150; one-hot [40, 24] Sigmoid (64-slot kernel) and log2 [48] ReLU (32-slot kernel).
    eval_step_budget = 16: every episode is suspended and resumed several times; then 4096: no suspension."""
    a, es, ps, tb = _deep_case(net, greedy)
    assert int(tb.lengths.median()) > 2 * 16 and int(tb.lengths.max()) > 4 * 16   # suspended, most several times
    try:
        for budget in (16, 4096):
            a.eval_step_budget = budget
            ev = a.evaluate_batch(es, ps, use_greedy=greedy)
            assert DEEP_EVAL in a.last_paths()["eval"]
            _assert_same(ev, tb)
    finally:
        del a.eval_step_budget


# ----------------------------------------------------------------------------------------------- 2. sized family
SIZED_CASES = [(3, "log2", [32], "ReLU"), (5, "onehot", [64, 32], "ReLU"), (8, "raw", [33], "Sigmoid")]


@pytest.mark.parametrize("case", SIZED_CASES, ids=[f"N{c[0]}-{c[1]}" for c in SIZED_CASES])
def test_sized_family_equals_its_trajectory_kernel(case):
    """N = 3 (W = 1), 5 (W = 2), 8 (W = 4) x the three obs modes, n = 70 (two full workgroups of 32 slots and a ragged
    one), eval_step_budget = 8.  max_steps = 40 as in tests/test_gpu_sized_rollout.py: random play on an 8 x 8 board
    does not end by itself in any reasonable time, so the large boards end by truncation -- after five suspensions --
    and the small one by termination."""
    size = case[0]
    a = _agent(*case, max_steps=40)
    a.use_fused_sized_rollout = True
    a.eval_step_budget = 8
    es, ps = _seeds(70, 21_000 + size)
    tb = a.rollout_batch(es, ps, use_greedy=False)
    assert a.last_paths()["rollout"].startswith("g2048_sized_rollout")
    ev = a.evaluate_batch(es, ps, use_greedy=False)
    assert SIZED_EVAL in a.last_paths()["eval"]
    W = int(a._lib.g2048_sized_words(size))
    assert tuple(ev.final_boards.shape) == (W, 70)
    assert int(tb.lengths.max()) > 2 * 8                # episodes were suspended at the budget, more than once
    assert int(tb.lengths.max()) == 40 if size > 3 else int(tb.lengths.min()) < 40
    _assert_same(ev, tb)


# ----------------------------------------------------------------------------------------------- 3. two-layer family
def test_two_layer_family_equals_its_trajectory_kernel():
    a = _agent(4, "log2", [40, 24], "ReLU", max_steps=64)
    es, ps = _seeds(100, 33_000)
    for greedy in (False, True):
        tb = a.rollout_batch(es, ps, use_greedy=greedy)
        assert a.last_paths()["rollout"].startswith("g2048_rollout ")
        ev = a.evaluate_batch(es, ps, use_greedy=greedy)
        assert FUSED_EVAL in a.last_paths()["eval"]
        _assert_same(ev, tb)
    assert int(tb.lengths.max()) == 64 and int(tb.lengths.min()) < 64    # truncated and terminated episodes


# ----------------------------------------------------------------------------------------------- 4. direct C calls
SENT64, SENT32, SENT8, PAD = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A, 0x5A, 37


def _direct(a, family, n, listed, es, ps, greedy=False):
    """One g2048_deep_eval / g2048_sized_eval call on `listed` (a strict subset of range(n)) with every output
    allocated PAD entries past its end and filled with a sentinel.  Returns the raw buffers."""
    from rl2048_amd import _lib as L
    from rl2048_amd.config import env_cfg_struct
    from rl2048_amd.vec_env import _as_u64_seeds

    lib, st = a._lib, a._stream
    W = int(lib.g2048_sized_words(a.size)) if family == "sized" else 1
    streams = []
    for seeds in (es, ps):
        sd = _as_u64_seeds(seeds, n, 0, DEV)
        s_, inc, buf = (torch.empty(2 * n, dtype=torch.int64, device=DEV), torch.empty(2 * n, dtype=torch.int64, device=DEV),
                        torch.empty(n, dtype=torch.int64, device=DEV))
        L.check(lib.g2048_seed_pcg64(L.ptr(sd), L.ptr(s_), L.ptr(inc), L.ptr(buf), n, st))
        streams += [s_, inc, buf]
    lengths = torch.full((n + PAD,), SENT32, dtype=torch.int32, device=DEV)
    totals = torch.full((n + PAD,), SENT64, dtype=torch.int64, device=DEV)           # fp64 bits
    max_e = torch.full((n + PAD,), SENT8, dtype=torch.uint8, device=DEV)
    final = torch.full((W * n + PAD,), SENT64, dtype=torch.int64, device=DEV)
    out = L.EvalOut(L.ptr(lengths), L.ptr(totals), L.ptr(max_e), L.ptr(final))
    sus_t = (torch.full((W * n + PAD,), SENT64, dtype=torch.int64, device=DEV),
             torch.full((3 * n + PAD,), SENT32, dtype=torch.int32, device=DEV),
             torch.full((n + PAD,), SENT64, dtype=torch.int64, device=DEV),
             torch.full((n + PAD,), SENT32, dtype=torch.int32, device=DEV),
             torch.zeros(1, dtype=torch.int32, device=DEV))
    sus = L.Suspend(*[L.ptr(t) for t in sus_t])
    queue = torch.zeros(1, dtype=torch.int32, device=DEV)
    order = torch.tensor(listed, dtype=torch.int32, device=DEV)
    cfg = env_cfg_struct(a.env_config)
    spec = a._deep_spec() if family == "deep" else a._sized_spec()
    _, hidden, act, harr = spec
    common = (len(hidden), harr, act, ctypes.byref(cfg), int(greedy), *[L.ptr(t) for t in streams], L.ptr(queue),
              L.ptr(order), len(listed), 0, ctypes.byref(sus), n, 1 << 20, ctypes.byref(out))
    if family == "deep":
        L.check(lib.g2048_deep_eval(L.ptr(a._pack_deep(a.params, spec, "actor", 4)), *common, st))
    else:
        L.check(lib.g2048_sized_eval(a.size, L.ptr(a._pack_sized(a.params, spec, "actor", 4)), *common, 0, st))
    torch.cuda.synchronize()
    assert int(sus_t[4].item()) == 0                    # nothing reaches 2^20 steps
    for t, s in zip(sus_t[:4], (SENT64, SENT32, SENT64, SENT32)):
        assert bool((t == s).all())                     # ... so the suspend state was not touched
    return W, lengths, totals, max_e, final


@pytest.mark.parametrize("family,case", [("deep", (4, "onehot", [40, 24], "Sigmoid")),
                                          ("deep", (4, "log2", [48], "ReLU")),
                                          ("sized", (5, "onehot", [64, 32], "ReLU"))],
                         ids=["deep64", "deep32", "sizedN5"])
def test_direct_calls_write_only_the_listed_episodes(family, case):
    """Sentinel tails past [n] (past [W, n] for the sized final board) and the entries of unlisted episodes are intact;
    the listed episodes got evaluate_batch's results (an episode depends on its own two seeds only)."""
    a = _agent(*case)
    a.use_fused_sized_rollout = family == "sized"
    n = 70
    es, ps = _seeds(n, 44_000)
    listed = [e for e in range(n) if e % 3 != 1][::-1]                   # a strict subset, not in order
    unl = torch.tensor([e for e in range(n) if e % 3 == 1], device=DEV)
    lis = torch.tensor(sorted(listed), device=DEV)
    W, lengths, totals, max_e, final = _direct(a, family, n, listed, es, ps)
    for buf, s in ((lengths, SENT32), (totals, SENT64), (max_e, SENT8)):
        assert bool((buf[n:] == s).all()) and bool((buf[unl] == s).all())
        assert not bool((buf[lis] == s).any())
    assert bool((final[W * n:] == SENT64).all())
    planes = final[:W * n].view(W, n)
    assert bool((planes[:, unl] == SENT64).all()) and not bool((planes[0, lis] == SENT64).any())
    ev = a.evaluate_batch(es, ps, use_greedy=False)
    assert torch.equal(lengths[lis], ev.lengths[lis])
    assert torch.equal(totals[lis], ev.total_reward.view(torch.int64)[lis])
    assert torch.equal(torch.ones_like(lis) << max_e[lis].long(), ev.max_tile[lis])
    fb = ev.final_boards if family == "sized" else ev.final_boards.view(1, n)
    assert torch.equal(planes[:, lis], fb[:, lis])


# ----------------------------------------------------------------------------------------------- 5. memory
def _peak_increase(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    r = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(DEV)
    del r
    return peak - base


def test_memory_does_not_depend_on_episode_length():
    """One-hot [40, 24], n = 4096: evaluate_batch's peak over the baseline is the same with max_steps 32 and 512, while
    rollout_batch's differs by at least the (512 - 32) rows of 18 B per episode it materialises -- so the comparison
    can see what it guards against."""
    n = 4096
    es, ps = _seeds(n, 55_000)
    inc = {}
    for ms in (32, 512):
        a = _agent(4, "onehot", [40, 24], "Sigmoid", max_steps=ms)
        w = _seeds(8, 1)
        a.evaluate_batch(*w)                            # warm-up: the packed net and the row table are allocated once
        a.rollout_batch(*w, use_greedy=True)
        inc[ms] = (_peak_increase(lambda: a.evaluate_batch(es, ps, use_greedy=False)),
                   _peak_increase(lambda: a.rollout_batch(es, ps, use_greedy=False)))
        assert DEEP_EVAL in a.last_paths()["eval"]
        del a
    print("peak increase (evaluate_batch, rollout_batch) by max_steps:", inc)
    assert inc[32][0] == inc[512][0]
    assert inc[512][1] - inc[32][1] >= (512 - 32) * 18 * n


# ----------------------------------------------------------------------------------------------- 6. bounded refusal
class _Counting:
    """The agent's library handle with the calls of the named entry points counted."""

    def __init__(self, lib, names):
        self._lib, self._names, self.calls = lib, (names,) if isinstance(names, str) else tuple(names), 0

    def __getattr__(self, k):
        fn = getattr(self._lib, k)
        if k not in self._names:
            return fn

        def counted(*args):
            self.calls += 1
            return fn(*args)

        return counted


@pytest.mark.parametrize("size,budget,limit,name,launches",
                         [(4, 4, 8, DEEP_EVAL, 2), (3, 2, 4, SIZED_EVAL, 2), (4, 100, 6, DEEP_EVAL, 1)],
                         ids=["4x4", "N3", "4x4-budget-past-the-limit"])
def test_bounded_refusal_after_exactly_two_launches(size, budget, limit, name, launches):
    """No game can end this early (a 4 x 4 board holds at most 10 tiles after 8 steps, a 3 x 3 board at most 6 after
    4), so every episode is still running when the next launch would pass eval_max_steps: two launches of
    eval_step_budget steps each.  A budget larger than eval_max_steps is cut to it: one launch, of 6 steps."""
    a = _agent(size, "onehot" if size == 4 else "log2", [40, 24] if size == 4 else [32], "ReLU")
    a.use_fused_sized_rollout = True
    a.eval_step_budget, a.eval_max_steps = budget, limit
    a._lib = _Counting(a._lib, name)
    n = 50
    with pytest.raises(RuntimeError, match=rf"{n} episode\(s\) still running.*max_steps") as ei:
        a.evaluate_batch(*_seeds(n, 66_000), use_greedy=False)
    assert a._lib.calls == launches
    assert f"after {limit} steps" in str(ei.value)
    assert "use_action_mask" not in str(ei.value)       # the mask is on: only max_steps is left to suggest
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------- 7. fall-through
FALL_CASES = {
    # a five-hidden-layer net: no persistent kernel covers it
    "five-layers-pcg64": ((4, "log2", [24, 24, 24, 24, 24], "ReLU"), "pcg64", True),
    # Philox streams: the persistent kernels are PCG64 only, so each family's own net must stay away from them
    "philox-deep-net": ((4, "onehot", [40, 24], "Sigmoid"), "philox", False),
    "philox-two-layer-net": ((4, "log2", [40, 24], "ReLU"), "philox", False),
    "philox-sized-net": ((3, "log2", [32], "ReLU"), "philox", False),
    "philox-five-layers": ((4, "log2", [24, 24, 24, 24, 24], "ReLU"), "philox", True),
}


@pytest.mark.parametrize("case", list(FALL_CASES))
def test_fall_through_materialises_rows_and_says_so(case):
    """What no score-only kernel covers goes through rollout_batch with the same rng: the same results, a path string
    that says rows were materialised and names rollout_batch's own path, and no call of a score-only entry point."""
    net, rng, greedy = FALL_CASES[case]
    a = _agent(*net, max_steps=48)                      # Philox draws need a finite max_steps
    a.use_fused_sized_rollout = True
    es, ps = _seeds(40, 77_000)
    tb = a.rollout_batch(es, ps, use_greedy=greedy, rng=rng)
    rollout_path = a.last_paths()["rollout"]
    assert "persistent" not in rollout_path             # the per-step paths
    a._lib = _Counting(a._lib, (FUSED_EVAL, DEEP_EVAL, SIZED_EVAL))
    ev = a.evaluate_batch(es, ps, use_greedy=greedy, rng=rng)
    assert a._lib.calls == 0
    assert a.last_paths()["eval"] == "rollout_batch (trajectory rows materialised): " + rollout_path
    assert a.last_paths()["rollout"] == rollout_path
    _assert_same(ev, tb)
    if rng == "philox" and case != "philox-five-layers":
        # the same agent on PCG64 streams does take its family's score-only kernel: the guard is the rng alone
        a.evaluate_batch(es, ps, use_greedy=greedy)
        assert a._lib.calls >= 1 and "no trajectory rows" in a.last_paths()["eval"]


def test_evaluate_batch_is_greedy_by_default():
    a = _agent(4, "onehot", [40, 24], "Sigmoid", max_steps=48)
    es, ps = _seeds(40, 78_000)
    _assert_same(a.evaluate_batch(es, ps), a.rollout_batch(es, ps, use_greedy=True))


# ----------------------------------------------------------------------------------------------- 8. runner
@pytest.mark.parametrize("greedy", [True, False], ids=["greedy", "sampled"])
def test_runner_score_only_summary_is_the_same(greedy):
    from rl2048_amd import runner as R

    a = _agent(4, "onehot", [40, 24], "Sigmoid")
    cfg = dict(num_episodes=64, env_base_seed=11, policy_base_seed=13, use_greedy=greedy)
    s0 = R.evaluation_loop(a, cfg, score_only=False)
    assert "eval" not in a.last_paths()
    s1 = R.evaluation_loop(a, cfg, score_only=True)
    assert DEEP_EVAL in a.last_paths()["eval"]
    assert s0 == s1 and s0["episodes"] == 64
