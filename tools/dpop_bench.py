"""DPOP on the GPU, measured: UTIL and VALUE timed apart with HIP events (mxs_dpop_stats reports the last
solve's two intervals), warm-up solves first, then the median and the spread over `--reps` solves.

    python tools/dpop_bench.py [--reps 9] [--warmup 3] [--fuse -1 0 128 512 2048] [--oracle]

Per instance and precision: entries/s of UTIL, launches, and the fraction of the HBM peak by ALGORITHMIC bytes
(every UTIL written once, every term table read once per use: a child's UTIL and a constraint table once by
the node that joins them).  `--fuse` lists the fuse_entries caps to compare (0 = one launch per level).
`--oracle` also times the numpy restatement (tests/dpop_oracle.py) on this host."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HBM_PEAK = 8.0e12     # bytes/s, MI355X


def algorithmic_bytes(g, eng, word):
    st = eng.stats()
    entries = st["total_entries"]
    tables = int(g.table_off[-1]) + int(g.dom_size.sum())
    return (2 * entries + tables) * word          # each UTIL written once and read once by its parent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fuse", type=int, nargs="+", default=[-1, 0])
    ap.add_argument("--oracle", action="store_true")
    args = ap.parse_args()
    from pydcop_amd import generators as G
    from pydcop_amd.dpop import DpopEngine, build_pseudotree
    from pydcop_amd.graph import Params
    cases = [("ising_grid(8, 128, seed=1)", G.ising_grid(8, 128, seed=1)),
             ("random_coloring(60, avg_degree=3, seed=4)", G.random_coloring(60, avg_degree=3, seed=4)),
             ("ising_grid(4, 12, seed=1)", G.ising_grid(4, 12, seed=1))]
    for name, g in cases:
        t0 = time.perf_counter()
        tree = build_pseudotree(g)
        t_tree = time.perf_counter() - t0
        for dtype in ("f64", "f32"):
            for fuse in args.fuse:
                with DpopEngine(g, Params(dtype=dtype), tree=tree, fuse_entries=fuse) as e:
                    for _ in range(args.warmup):
                        e.solve()
                    util, value = [], []
                    for _ in range(args.reps):
                        e.solve()
                        st = e.stats()
                        util.append(st["util_ns"] * 1e-3)
                        value.append(st["value_ns"] * 1e-3)
                    u, v = statistics.median(util), statistics.median(value)
                    word = 4 if dtype == "f32" else 8
                    row = {"instance": name, "dtype": dtype, "fuse_entries": fuse, "tree_s": round(t_tree, 4),
                           "util_us": round(u, 1), "util_us_min_max": [round(min(util), 1), round(max(util), 1)],
                           "value_us": round(v, 1), "value_us_min_max": [round(min(value), 1), round(max(value), 1)],
                           "launches_util": st["launches_util"], "launches_value": st["launches_value"],
                           "total_entries": st["total_entries"], "depth": st["depth"],
                           "util_entries_per_s": round(st["total_entries"] / (u * 1e-6), 0),
                           "util_hbm_fraction": round(algorithmic_bytes(g, e, word) / (u * 1e-6) / HBM_PEAK, 4),
                           "reps": args.reps, "warmup": args.warmup}
                    print(json.dumps(row), flush=True)
        if args.oracle:
            from dpop_oracle import OracleDpop
            t0 = time.perf_counter()
            OracleDpop(g, Params(), tree=tree).solve()
            print(json.dumps({"instance": name, "numpy_oracle_s": round(time.perf_counter() - t0, 3),
                              "host_cpus": os.cpu_count()}), flush=True)


if __name__ == "__main__":
    main()
