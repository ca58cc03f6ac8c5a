"""TOOL: time g2048_sized_step on the GPU box (board sizes other than 4).

    python tools/bench_sized.py [--lanes 1048576] [--launches 200] [--out profiles/sized/bench_sized.json]

Per case: one HIP event pair around every launch, `--launches` launches after 20 warm-up launches, median and
p10 / p90 of the per-launch times; the bytes per board-step counted from the buffers the launch touches, the achieved
bytes per second, and as the yardstick a float4 copy (tools/membench.hip) of the same number of bytes on the same box.
Cases: N in {3, 5, 8} x {PCG64 + log2 obs + packed mask, Philox without obs}; for information the sized kernel at
N = 4 next to step_kernel (g2048_step) in the same run.  Lanes auto-reset, so every launch steps every lane.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libmembench.so")


def bytes_per_step(size: int, rng: str, obs: bool) -> dict:
    """Bytes one board-step reads / writes, from the buffers g2048_sized_step touches (packed mask, fp32 reward)."""
    W = (size * size + 15) // 16
    rd = 8 * W + 4 + 1                      # board planes, state word, action
    wr = 8 * W + 4 + 4 + 1 + 1              # board planes, state word, reward, flags, mask byte
    if rng == "pcg64":
        rd += 16 + 16 + 4                   # PCG64 state, increment, uint32 buffer
        wr += 16 + 4                        # state and buffer written back
    else:
        rd += 8                             # the lane seed (Philox counter)
    if obs:
        wr += 4 * size * size               # log2 obs
    return {"read": rd, "write": wr, "total": rd + wr}


def time_launches(fn, launches: int, warmup: int = 20) -> dict:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    us = np.array([s.elapsed_time(e) * 1e3 for s, e in ev])
    return {"median_us": float(np.median(us)), "p10_us": float(np.percentile(us, 10)),
            "p90_us": float(np.percentile(us, 90)), "launches": launches}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=1 << 20)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sized", "bench_sized.json"))
    a = ap.parse_args()
    from rl2048_amd import Game2048EnvConfig, VecGame2048Env

    if not os.path.exists(SO):
        subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-shared", "-fPIC", "-o", SO,
                        os.path.join(HERE, "membench.hip")], check=True)
    MB = ctypes.CDLL(SO)
    dev = torch.device("cuda", 0)
    n = a.lanes
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cpu").manual_seed(1)
    actions = torch.randint(0, 4, (n,), generator=g, dtype=torch.uint8).to(dev)

    def copy_yardstick(total_bytes: int) -> dict:
        nb = (total_bytes // 2) & ~15
        src = torch.zeros(nb, dtype=torch.uint8, device=dev)
        dst = torch.zeros(nb, dtype=torch.uint8, device=dev)
        t = time_launches(lambda: MB.mb_copy(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()),
                                             ctypes.c_size_t(nb // 16), 4096, ctypes.c_void_p(stream)), a.launches)
        t["bytes"] = 2 * nb
        t["GBs"] = 2 * nb / t["median_us"] / 1e3
        return t

    def env_case(size: int, rng: str, obs: bool, sized4: bool = False) -> dict:
        cfg = Game2048EnvConfig(size=size, obs_mode="log2", obs_log2_scale=0.0625, reward_mode="log2",
                                base_reward_scale=0.5, max_steps=1024)
        env = VecGame2048Env(n, cfg, device=dev, rng=rng, auto_reset=True, track_score=False, packed_mask=True)
        if sized4:      # the sized kernel on 4 x 4 boards (W = 1): same buffers, the sized entry points
            env._sized = True
            env.board = env.board.view(1, n)
            env._out = env._sized_out(env.reward, env.flags, None, True, None)
        env.reset(seed=7)
        t = time_launches(lambda: env.step_into(actions, write_obs=obs), a.launches)
        b = bytes_per_step(size, rng, obs)
        t.update(size=size, rng=rng, obs="log2" if obs else "none", lanes=n, bytes_per_board_step=b,
                 kernel="g2048_sized_step" if (size != 4 or sized4) else "g2048_step",
                 GBs=b["total"] * n / t["median_us"] / 1e3, board_steps_per_s=n / t["median_us"] * 1e6)
        t["copy_yardstick"] = copy_yardstick(b["total"] * n)
        t["fraction_of_copy"] = t["GBs"] / t["copy_yardstick"]["GBs"]
        return t

    out = {"device": torch.cuda.get_device_name(0), "cases": [], "size4_for_information": []}
    for size in (3, 5, 8):
        out["cases"].append(env_case(size, "pcg64", True))
        out["cases"].append(env_case(size, "philox", False))
    for sized4 in (False, True):
        out["size4_for_information"].append(env_case(4, "pcg64", True, sized4))
        out["size4_for_information"].append(env_case(4, "philox", False, sized4))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for c in out["cases"] + out["size4_for_information"]:
        print(json.dumps({k: c[k] for k in ("kernel", "size", "rng", "obs", "median_us", "p10_us", "p90_us", "GBs",
                                            "fraction_of_copy")} | {"B_per_board_step": c["bytes_per_board_step"]["total"]}),
              flush=True)


if __name__ == "__main__":
    sys.exit(main())
