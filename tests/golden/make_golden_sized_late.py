"""Generate the late-game board-size fixture (sizes 2..8, 4 included) from the REAL reference (build container only).

    python tests/golden/make_golden_sized_late.py [--ref /root/reference]

Imports the reference's own modules like make_golden_sized.py (``import_reference`` + tests/golden/gym_shim/), runs
them unchanged and writes tests/golden/sized_late.npz (data only).  sized.npz holds random play from reset, cut at 60
steps for N >= 5: no termination, no nearly full board, no exponent above 6 at those sizes.  This file starts the
reference on crafted boards instead -- the families of tests/sized_ref.py::family_boards (dense high tiles, explicit
14 / 15 lines in the word-straddling rows, one empty cell at the word edges, terminal and near-terminal
checkerboards, boards that fill the merged list):

  for every N in 2..8, config c in ENV_SEL and family board:  env.reset(seed); env.game.board = board; then steps with
  an action drawn uniformly among the valid ones (any action when none is valid) until terminated, truncated or 24
  steps.

A 2^15 + 2^15 merge makes the reference hold 65536 (exponent 16), which the kernels' nibble boards cannot: that step
is recorded as the reference gave it (boards and merged lists may hold 16), the episode is marked ``ep_sat`` and ends
there.

  n{N}_fam            family name of every episode's board (the same boards under every config)
  n{N}_c{c}_ep_*      seed, start, len, board (the injected board), sat
  n{N}_c{c}_<field>   per step, as sized.npz: action, board, reward (fp64), terminated, truncated, invalid,
                      max_tile_seen, score, step_index, mask, merged.  No obs: it is a pure function of the board.

Boards are uint8 exponents [..., N*N]; merged lists uint8 exponents padded with zeros to N*(N//2).
The coverage the GPU tests rely on is asserted here before the file is written (and again, on the committed file, by
tests/test_sized_ref_cpu.py).
"""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import seed_iter  # noqa: E402
from make_golden_ref import ENV_CFGS, import_reference  # noqa: E402
from make_golden_sized import ENV_SEL, exps, mask_bits, pad_merged, vals  # noqa: E402
from sized_ref import family_boards, late_coverage, late_coverage_ok  # noqa: E402

SIZES = [2, 3, 4, 5, 6, 7, 8]
MAX_LEN = 24
FAMILY_SEED = 2048


def gen(E, data):
    rng = np.random.default_rng(8192)
    it = seed_iter(29)
    data["env_cfgs"] = np.array(json.dumps({str(c): ENV_CFGS[c] for c in ENV_SEL}))
    for n in SIZES:
        fam = family_boards(n, FAMILY_SEED)
        data[f"n{n}_fam"] = np.array([name for name, _ in fam])
        for c in ENV_SEL:
            env = E.Game2048Env(E.Game2048EnvConfig(size=n, **ENV_CFGS[c]))
            keys = ("action", "board", "reward", "terminated", "truncated", "invalid", "max_tile_seen", "score",
                    "step_index", "mask", "merged")
            st = {k: [] for k in keys}
            ep = {k: [] for k in ("seed", "start", "len", "board", "sat")}
            for name, board in fam:
                seed = next(it)
                env.reset(seed=seed)
                env.game.board = vals(board).reshape(n, n)
                ep["seed"].append(seed)
                ep["start"].append(len(st["action"]))
                ep["board"].append(board)
                t, sat = 0, False
                while t < MAX_LEN:
                    valid = [i for i, v in enumerate(env.game.get_action_mask()) if v]
                    a = int(valid[int(rng.integers(len(valid)))]) if valid else int(rng.integers(4))
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
                    st["merged"].append(pad_merged(info["merged"], n))
                    t += 1
                    sat = 65536 in info["merged"]
                    if term or trunc or sat:
                        break
                ep["len"].append(t)
                ep["sat"].append(sat)
            p = f"n{n}_c{c}_"
            data[p + "ep_seed"] = np.array(ep["seed"], dtype=np.uint64)
            data[p + "ep_start"] = np.array(ep["start"], dtype=np.int64)
            data[p + "ep_len"] = np.array(ep["len"], dtype=np.int64)
            data[p + "ep_board"] = np.array(ep["board"], dtype=np.uint8)
            data[p + "ep_sat"] = np.array(ep["sat"], dtype=np.bool_)
            dt = dict(action=np.uint8, board=np.uint8, reward=np.float64, terminated=np.bool_, truncated=np.bool_,
                      invalid=np.bool_, max_tile_seen=np.int64, score=np.int64, step_index=np.int64, mask=np.uint8,
                      merged=np.uint8)
            for k, v in st.items():
                data[p + k] = np.array(v, dtype=dt[k])
            print(f"  size {n} cfg {c}: {len(fam)} episodes, {len(st['action'])} steps, "
                  f"{int(np.sum(st['terminated']))} terminated, {int(np.sum(ep['sat']))} saturated")
        cov = late_coverage(data, n)
        print(f"  size {n} coverage: {cov}")
        assert late_coverage_ok(cov, n), (n, cov)


def save_npz(path, data):
    """np.savez_compressed with fixed member times: the same data gives the same bytes on every run."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in data.items():
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    E, _, _ = import_reference(args.ref)
    data = {"sizes": np.array(SIZES), "env_sel": np.array(ENV_SEL)}
    gen(E, data)
    out = os.path.join(HERE, "sized_late.npz")
    save_npz(out, data)
    print("wrote", out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < (1 << 20), "committed files stay below 1 MiB: fewer boards per family, not families"


if __name__ == "__main__":
    main()
