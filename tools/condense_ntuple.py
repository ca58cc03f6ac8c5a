"""TOOL: condense outputs of tools/train_ntuple.py and tools/bench_ntuple.py into the small files kept under
profiles/ntuple/ (the tools write one record per evaluation / per call, tens of thousands of lines per run).

    python tools/condense_ntuple.py --train NAME=train.json [NAME=...] --out-train profiles/ntuple/train_ntuple.json
    python tools/condense_ntuple.py --bench TAG=bench.json [TAG=...] [--update TAG=bench.json ...]
                                    --out-bench profiles/ntuple/bench_ntuple.json

train: per run the settings, a summary over ALL its evaluations (first / last / lowest / highest mean score, rows,
seconds, the last max-tile histogram, the final greedy and depth-1 scores) and 24 evenly spaced evaluations as
[iteration, mean score, mean length].  bench: one line per case "TAG:case" with M env steps/s as [median, min, max] and
every timed call's seconds for both players; `updates`: the "update" section of each --update file (default: of every
--bench file) the same way.  Nothing is recomputed: every number is the tools', rounded.
"""
import argparse
import json


def one_line(obj):
    return json.dumps(obj, separators=(", ", ": "))


def dump(path, top, lines_key, rows):
    """A dict `top` plus `lines_key` -> {name: row}, one row per line."""
    with open(path, "w") as f:
        f.write("{\n")
        for k, v in top.items():
            f.write(f" {json.dumps(k)}: {one_line(v)},\n")
        f.write(f" {json.dumps(lines_key)}: {{\n")
        items = list(rows.items())
        for i, (k, v) in enumerate(items):
            f.write(f"  {json.dumps(k)}: {one_line(v)}{',' if i + 1 < len(items) else ''}\n")
        f.write(" }\n}\n")
    with open(path) as f:
        json.load(f)


def pairs(items):
    return [tuple(x.split("=", 1)) for x in items or []]


def load(path):
    with open(path) as f:
        return json.load(f)


def condense_train(named, out):
    runs, d = {}, None
    for name, path in named:
        d = load(path)
        c = d["curve"]
        sc = [x["mean_score"] for x in c]
        idx = sorted(set(round(i * (len(c) - 1) / 23) for i in range(24)))
        score = lambda v: {k: (round(v[k], 1) if k != "share_2048" else v[k])              # noqa: E731
                           for k in ("mean_score", "mean_length", "share_2048")}
        runs[name] = {
            "episodes": d["episodes"], "lr_num": d["lr_num"], "lr_shift": d["lr_shift"], "iterations": d["iterations"],
            "evaluations": len(c), "rows_trained": c[-1]["rows_trained"],
            "train_seconds": round(c[-1]["train_seconds"], 1), "mean_score_first": round(sc[0], 1),
            "mean_score_last": round(sc[-1], 1), "mean_score_min": round(min(sc), 1),
            "mean_score_max_after_first": round(max(sc[1:]), 1), "share_2048_max": max(x["share_2048"] for x in c),
            "max_tile_counts_last": c[-1]["max_tile_counts"],
            "final": {k: (v if k == "episodes" else score(v)) for k, v in d["final"].items()},
            "curve_iteration_meanscore_meanlength": [[c[i]["iteration"], round(c[i]["mean_score"]),
                                                      round(c[i]["mean_length"])] for i in idx]}
    top = {"tool": "tools/train_ntuple.py, condensed by tools/condense_ntuple.py", "device": d["device"],
           "size": d["size"], "depth": 0, "eval_episodes": d["eval_episodes"], "features": d["features"],
           "weights": d["weights"], "recorded_expectimax_means": d["recorded_expectimax_means"]}
    dump(out, top, "runs", runs)


def condense_bench(named, updates, out):
    cases, ups, d = {}, {}, None
    for tag, path in named:
        d = load(path)
        for k, r in d["cases"].items():
            row = {"weights": d["weights"], "warmup": r["warmup"]}
            for w in ("ntuple", "expectimax"):
                p = r[w]
                row[w] = {"M_steps_per_s_median_min_max": [round(p[f"steps_per_s_{s}"] / 1e6, 4)
                                                           for s in ("median", "min", "max")],
                          "time_s_calls": [round(c["time_s"], 5) for c in p["calls"]], "steps": p["steps"],
                          "mean_total_reward": round(p["mean_total_reward"], 1),
                          "mean_length": round(p["mean_length"], 1), "share_2048": p["share_2048"]}
            row["ntuple_over_expectimax"] = round(r["steps_per_s_ntuple_over_expectimax"], 4)
            cases[f"{tag}:{k}"] = row
    for tag, path in updates or named:
        b = load(path)
        u = b["update"]
        row = {"weights": b["weights"]}
        row.update({k: (round(v, 5) if isinstance(v, float) else v) for k, v in u.items() if not isinstance(v, dict)})
        for w in ("played", "random_fills"):
            p = u[w]
            row[w] = {"M_rows_per_s_median_min_max": [round(p[f"rows_per_s_{s}"] / 1e6, 3) for s in ("median", "min", "max")],
                      "time_s_calls": [round(c["time_s"], 5) for c in p["calls"]], "rows": p["rows"],
                      "abs_delta": p["abs_delta"], "weights_changed": p["weights_changed"]}
        ups[tag] = row
    top = {"tool": "tools/bench_ntuple.py, condensed by tools/condense_ntuple.py", "device": d["device"],
           "calls": d["calls"], "calls_deep": d["calls_deep"], "warmup": d["warmup"], "updates": ups}
    dump(out, top, "cases", cases)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", nargs="*")
    ap.add_argument("--out-train")
    ap.add_argument("--bench", nargs="*")
    ap.add_argument("--update", nargs="*")
    ap.add_argument("--out-bench")
    a = ap.parse_args()
    if a.train:
        condense_train(pairs(a.train), a.out_train)
    if a.bench:
        condense_bench(pairs(a.bench), pairs(a.update), a.out_bench)


if __name__ == "__main__":
    main()
