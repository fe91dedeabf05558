"""Summarise a `rocprofv3 --kernel-trace --stats` database of `backward_bench.py --step-only` runs.

    rocprofv3 --kernel-trace --stats -d OUT/<net> -o run -- python profiles/backward_bench.py --step-only --net <net> \
        --mode composite --batch 128 --steps 1
    python profiles/backward_profile_summary.py OUT/<net>/run_results.db [...] > profiles/backward_baseline_profile.json

A --step-only run executes 4 identical steps (2 warm-up, 2 timed).  The last quarter of the dispatches (by start time) is
one steady-state step: its kernel time by category, its launch count, and the idle time between its first start and its
last end.
"""
import json
import sqlite3
import sys

CATEGORIES = (
    ("miopen_conv", ("conv", "miopen", "igemm", "gemm", "winograd", "Cijk")),
    ("batchnorm", ("BatchNorm", "batch_norm")),
    ("slfp_hip", ("slfp", "k_")),
    ("aten_elementwise_reduce", ("elementwise", "vectorized", "reduce", "Reduce", "fill", "copy", "index", "softmax",
                                 "nll", "mean", "sum", "unrolled", "Relu", "relu", "threshold")),
)


def category(name):
    for cat, keys in CATEGORIES:
        if any(k in name for k in keys):
            return cat
    return "other"


def summarise(db, steps=4):
    c = sqlite3.connect(db)
    rows = c.execute("select name, start, end, duration from kernels order by start").fetchall()
    n = len(rows) // steps
    last = rows[-n:]
    span_ns = last[-1][2] - last[0][1]
    busy_ns = sum(r[3] for r in last)
    cats, kern = {}, {}
    for name, _, _, d in last:
        k = category(name)
        cats[k] = cats.get(k, 0) + d
        short = name.split("(")[0][:90]
        e = kern.setdefault(short, [0, 0])
        e[0] += 1
        e[1] += d
    top = sorted(kern.items(), key=lambda kv: -kv[1][1])[:15]
    return {
        "db": db.split("/")[-2],
        "launches_per_step": n,
        "step_span_ms": round(span_ns / 1e6, 3),
        "kernel_busy_ms": round(busy_ns / 1e6, 3),
        "idle_between_kernels_ms": round((span_ns - busy_ns) / 1e6, 3),
        "by_category_ms": {k: round(v / 1e6, 3) for k, v in sorted(cats.items(), key=lambda kv: -kv[1])},
        "top_kernels": [{"name": k, "calls": v[0], "ms": round(v[1] / 1e6, 3)} for k, v in top],
    }


if __name__ == "__main__":
    print(json.dumps([summarise(p) for p in sys.argv[1:]], indent=1))
