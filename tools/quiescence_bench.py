"""What Max-Sum's device-side quiescence check costs (MaxSumEngine.watch_quiescence), on the MI355X, in one process:

  (a) plain run                      (b) watch_quiescence(1)         (c) watch_quiescence(10)
  (d) the host loop run(k) + messages() for k = 1 and 10 -- the only way to decide the same thing before: copy all
      messages and counters back and look at the counters
  (p1, p2) plain run on ANOTHER build of the library (--parent-lib: the parent commit's), twice: their difference is
           the spread that (a) is judged against -- watching off must cost nothing

on random_coloring(100_000) f64 (the benchmark's instance: eager launches) and random_coloring(10_000), with the default
schedule (eager too) and with graph_chunk = 32 (32-cycle graph replay).  Every figure is host wall time per cycle of a
synchronous call (`run` waits for the stream), in microseconds: the median of --reps alternating repetitions of --cycles
cycles after one warm-up round of the same shapes.  Last, on the 100k instance: the wall time of
run_until_quiescent(cap) from cycle 0 against run(cap) with the same cap, and the detected cycle.  One JSON document on
stdout, and in --out.

    python tools/quiescence_bench.py --parent-lib /path/to/libmaxsum_hip_parent.so --out profiles/quiescence_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pydcop_amd import generators as G  # noqa: E402
from pydcop_amd.engine import MaxSumEngine  # noqa: E402
from pydcop_amd.graph import Params  # noqa: E402


def timed(fn, cycles):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6 / cycles


def host_loop(eng, cycles, k):
    for _ in range(cycles // k):
        eng.run(k)
        _, _, cv, cf = eng.messages()
        bool((cv == 4).all() and (cf == 4).all())


def bench(name, graph, cycles, reps, parent_lib, graph_chunk=-1):
    configs = {}

    def add(key, every=None, loop=None, lib=None):
        eng = MaxSumEngine(graph, Params(graph_chunk=graph_chunk), lib_path=lib)
        if every:
            eng.watch_quiescence(every)
        configs[key] = (eng, (lambda: host_loop(eng, cycles, loop)) if loop else (lambda: eng.run(cycles)))

    add("a_plain")
    add("b_watch_1", every=1)
    add("c_watch_10", every=10)
    add("d_host_loop_1", loop=1)
    add("d_host_loop_10", loop=10)
    if parent_lib:
        add("p1_parent_plain", lib=parent_lib)
        add("p2_parent_plain", lib=parent_lib)
    for _, fn in configs.values():          # warm-up: the same shapes (builds the graphs too)
        fn()
    times = {k: [] for k in configs}
    for _ in range(reps):                   # alternating
        for k, (_, fn) in configs.items():
            times[k].append(timed(fn, cycles))
    any_eng = configs["a_plain"][0]
    row = {"instance": name, "n_vars": graph.n_vars, "n_factors": graph.n_factors, "n_edges": graph.n_edges,
           "cycles": cycles, "reps": reps,
           "bytes_per_cycle": any_eng.cycle_bytes()[0], "launches_per_cycle": any_eng.cycle_bytes()[1],
           "launches_per_check": 2,
           "graph_chunk": graph_chunk,     # -1: the default (32-cycle replay below 4 MB per cycle, eager above)
           "graph_replay": graph_chunk >= 2 or (graph_chunk < 0 and any_eng.cycle_bytes()[0] < (4 << 20)),
           "us_per_cycle": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}}
    if parent_lib:
        m = row["us_per_cycle"]
        row["parent_spread_us"] = abs(m["p1_parent_plain"]["median"] - m["p2_parent_plain"]["median"])
        row["plain_minus_parent_us"] = m["a_plain"]["median"] - min(m["p1_parent_plain"]["median"], m["p2_parent_plain"]["median"])
    row["quiescence_b"] = configs["b_watch_1"][0].quiescence()
    row["quiescence_c"] = configs["c_watch_10"][0].quiescence()
    for eng, _ in configs.values():
        eng.close()
    return row


def until_quiescent(name, graph, cap, reps):
    """run_until_quiescent(cap) from cycle 0 against run(cap): wall time of the whole call, milliseconds"""
    out = {"instance": name, "cap": cap, "reps": reps, "run_until_quiescent_ms": [], "run_cap_ms": []}
    with MaxSumEngine(graph, Params()) as watched, MaxSumEngine(graph, Params()) as plain:
        watched.watch_quiescence(1)
        for rep in range(reps + 1):         # (the first round warms up)
            watched.reset(), plain.reset()
            t0 = time.perf_counter()
            r = watched.run_until_quiescent(cap)
            t1 = time.perf_counter()
            plain.run(cap)
            t2 = time.perf_counter()
            if rep:
                out["run_until_quiescent_ms"].append((t1 - t0) * 1e3)
                out["run_cap_ms"].append((t2 - t1) * 1e3)
        out["result"] = r
        out["quiescence"] = watched.quiescence()
    for k in ("run_until_quiescent_ms", "run_cap_ms"):
        out[k] = {"median": statistics.median(out[k]), "min": min(out[k]), "max": max(out[k])}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cycles", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cap", type=int, default=2000, help="the cap of the run_until_quiescent comparison")
    ap.add_argument("--parent-lib", default=None, help="another build of libmaxsum_hip (name starts with libmaxsum_hip)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.cycles < 10 or args.cycles % 10 or args.reps < 1:
        raise SystemExit("--cycles: a multiple of 10; --reps >= 1")
    big = G.random_coloring(100_000)
    rows = [bench("coloring_100k_f64", big, args.cycles, args.reps, args.parent_lib),
            bench("coloring_10k_f64", G.random_coloring(10_000), args.cycles, args.reps, args.parent_lib),
            bench("coloring_10k_f64_replay32", G.random_coloring(10_000), args.cycles, args.reps, args.parent_lib, graph_chunk=32)]
    doc = {"tool": "tools/quiescence_bench.py", "unit": "microseconds of host wall time per cycle", "rows": rows,
           "until_quiescent": until_quiescent("coloring_100k_f64", big, args.cap, args.reps)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
