"""GPU: bench.py --dump-outputs writes what the last step returned, for every lane or a fixed sample of them."""
import argparse
import os

import numpy as np
import pytest
import torch

import bench

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _stepped_env(n, obs, rng="pcg64", steps=3):
    args = argparse.Namespace(rng=rng, obs=obs, no_auto_reset=False, gpus=1)
    env = bench.make_env(torch, args, n, 0, DEV)
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    actions = torch.randint(0, 4, (steps, n), dtype=torch.uint8, device=DEV, generator=g)
    for k in range(steps):
        env.step_into(actions[k])
    return env


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("obs,rng", [("log2", "pcg64"), ("onehot", "philox"), ("none", "pcg64")])
def test_dump_holds_every_lane_of_the_last_step(tmp_path, obs, rng):
    n = 4099
    env = _stepped_env(n, obs, rng)
    info = bench.dump_outputs(torch, env, str(tmp_path / "d"), obs != "none")
    got = _load(tmp_path / "d")
    assert set(got) == {"lanes", "reward", "flags", "action_mask", "board"} | ({"obs"} if obs != "none" else set())
    assert info["lanes"] == info["of"] == n and info["bytes"] == sum(a.nbytes for a in got.values())
    assert got["lanes"].dtype == np.float64 and all(a.dtype == np.float32 for k, a in got.items() if k != "lanes")
    np.testing.assert_array_equal(got["lanes"], np.arange(n))
    np.testing.assert_array_equal(got["reward"], env.reward.cpu().numpy())
    np.testing.assert_array_equal(got["flags"], env.flags.cpu().numpy())
    np.testing.assert_array_equal(got["action_mask"], env.action_mask.cpu().numpy())
    np.testing.assert_array_equal(got["board"], env.boards_exponents().view(n, 16).cpu().numpy())
    if obs != "none":
        np.testing.assert_array_equal(got["obs"], env.obs.cpu().numpy())
        assert got["obs"].shape == (n, env.obs_width)


def test_dump_samples_the_same_lanes_when_over_budget(tmp_path, monkeypatch):
    n = 4099
    per_lane = 4 * (1 + 1 + 4 + 16 + 16) + 8
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1000 * per_lane + 5)
    a = bench.dump_outputs(torch, _stepped_env(n, "log2"), str(tmp_path / "a"), True)
    b = bench.dump_outputs(torch, _stepped_env(n, "log2"), str(tmp_path / "b"), True)
    assert a["lanes"] == 1000 and a["bytes"] <= 1000 * per_lane + 5 and a["bytes"] == b["bytes"]
    ga, gb = _load(tmp_path / "a"), _load(tmp_path / "b")
    lanes = ga["lanes"].astype(np.int64)
    assert len(np.unique(lanes)) == 1000 and (np.diff(lanes) > 0).all() and 0 <= lanes[0] and lanes[-1] < n
    for k in ga:                       # two runs from the same inputs: the same lanes, the same values
        np.testing.assert_array_equal(ga[k], gb[k])
    env = _stepped_env(n, "log2")
    np.testing.assert_array_equal(ga["reward"], env.reward.cpu().numpy()[lanes])
    np.testing.assert_array_equal(ga["obs"], env.obs.cpu().numpy()[lanes])
