"""TOOL: the rollout legs of `bench.py --full`, rollout_batch alone, with each call's time split at the persistent
launch (GPU box).

    python tools/bench_rollout_legs.py [--calls 7] [--out profiles/rollout_driver/legs.json]

Four legs in ONE process, alternating, as bench.py's training-iteration legs meet them: configs[1] at 65,536 and
configs[2] at 1,048,576 episodes (g2048_rollout), the runner's documented config at both sizes (g2048_deep_rollout,
max_steps None).  One warm-up round, then `--calls` rounds.  Per call: wall time (host clock, synchronise before and
after, as bench.py), the device time of the persistent launch alone (events round the C call), the device time from
the call's start to that launch and from its end to the call's end (what the host driver adds shows there), and the
caching allocator's device allocations during the call (0 once warm: a call that reaches hipMalloc is timing that).
Run it on two checkouts alternately to compare them; kernel time between two processes of the same code differs by a
few tenths of a millisecond, so the split says whether a difference is the host's."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class TimedLaunches:
    """The library with events round the named entry points."""

    def __init__(self, lib, names):
        self._lib, self._names, self.events = lib, names, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in self._names:
            return fn

        def timed(*args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*args)
            e1.record()
            self.events.append((e0, e1))
            return rc
        return timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_driver", "legs.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rollout_legs needs a HIP device: a timing taken elsewhere says nothing")
    import bench
    from rl2048_amd import Game2048EnvConfig
    from rl2048_amd.agent import ReinforceAgent, ReinforceAgentConfig
    from rl2048_amd.mlp import MLPConfig

    dev = torch.device("cuda", 0)
    c1 = ReinforceAgent(Game2048EnvConfig(), MLPConfig(hidden_sizes=[256, 256], activation="ReLU",
                                                       init_distribution="HeNormal"),
                        ReinforceAgentConfig(baseline_mode="batch"), device=dev)
    ref = ReinforceAgent(Game2048EnvConfig(**bench.REFCONF_ENV), MLPConfig(**bench.REFCONF_MLP),
                         ReinforceAgentConfig(**bench.REFCONF_AGENT), device=dev)
    lib = TimedLaunches(c1._lib, ("g2048_rollout", "g2048_deep_rollout"))
    c1._lib = ref._lib = lib
    legs = {"configs1_65536": (c1, 1 << 16), "configs2_1048576": (c1, 1 << 20),
            "refconfig_65536": (ref, 1 << 16), "refconfig_1048576": (ref, 1 << 20)}
    res = {k: {"wall_ms": [], "kernel_ms": [], "before_ms": [], "after_ms": [], "device_allocations": []} for k in legs}
    for rep in range(a.calls + 1):
        for name, (agent, n) in legs.items():
            es = np.arange(1000 + rep * n, 1000 + (rep + 1) * n, dtype=np.int64)
            ps = es + 7 * n
            torch.cuda.synchronize()
            segments = torch.cuda.memory_stats(dev)["segment.all.allocated"]
            lib.events.clear()
            b0, b1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            b0.record()
            b = agent.rollout_batch(es, ps)
            b1.record()
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            if rep:
                r = res[name]
                r["wall_ms"].append(wall * 1e3)
                r["kernel_ms"].append(sum(x.elapsed_time(y) for x, y in lib.events))
                r["before_ms"].append(b0.elapsed_time(lib.events[0][0]))
                r["after_ms"].append(lib.events[-1][1].elapsed_time(b1))
                r["device_allocations"].append(int(torch.cuda.memory_stats(dev)["segment.all.allocated"] - segments))
            res[name]["path"] = agent.last_paths()["rollout"]
            res[name]["env_steps"] = int(b.lengths.sum())
            del b
    for name, r in res.items():
        print("%-18s wall %.3f  launch %.3f  before %.3f  after %.3f ms  device allocations %d  (%s)" % (
            name, np.median(r["wall_ms"]), np.median(r["kernel_ms"]), np.median(r["before_ms"]),
            np.median(r["after_ms"]), sum(r["device_allocations"]), r["path"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "calls": a.calls, "legs": res}, f, indent=1)


if __name__ == "__main__":
    main()
