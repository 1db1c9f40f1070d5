"""Cycles per second of the DSA, MGM and MGM-2 engines (pydcop_amd/csrc/dsa.hip, mgm.hip, mgm2.h) on the
100k-variable colouring instance of the bench and on the meeting instance (24 values, arity 3):

    python tools/local_search_bench.py [--cycles 500] [--mgm2-rounds 200] [--gdba-rounds 200] [--dba-rounds 200]

One JSON line per (algorithm, instance, kernels); "kernels": "packed" = the default (lane per
constraint where the instance allows it, local_search.h), "slots" = the thread-per-variable
register-array kernels on the slot view (MAXSUM_LOCAL_SEARCH_GENERIC=2), "csr_walk" = the generic
kernels (=1), "strided" = the default kernels without the private row copies of the variables the pack
cannot take (MAXSUM_LOCAL_SEARCH_ROWS=0: their D entries per constraint a stride apart, round 3).
MGM-2 has one family of kernels ("kernels": "mgm2"), timed in f64 and f32 after the MGM / DSA rows of an
instance.  GDBA ("kernels": "gdba", pydcop_amd/csrc/gdba.h) follows, in f64 and f32, increase modes E and C (the
heaviest mode with live tables): the median of three timed runs after a warm-up, next to an MGM row timed the same
way in the same precision (both tagged "timing": "median3"; "ratio_to_mgm"), with the bytes the engine keeps on the device for the share of the HBM
peak; every timing ends with the engine's stream synchronised (run() returns after it).
`--dba-rounds N` (default 0) prints three rows instead, timed the same way in one process on the hard 100k-variable
3-colouring: DBA ("kernels": "dba", pydcop_amd/csrc/dba.h; `infinity: 1000`, `max_distance` above the round count so
that nothing stops), GDBA (A, NZ, T, f64) and MGM (f64), with DBA's ratio to each.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from pydcop_amd import generators as G  # noqa: E402
from pydcop_amd.dsa import DsaEngine  # noqa: E402
from pydcop_amd.gdba import GdbaEngine  # noqa: E402
from pydcop_amd.graph import Params  # noqa: E402
from pydcop_amd.mgm import MgmEngine  # noqa: E402
from pydcop_amd.mgm2 import Mgm2Engine  # noqa: E402


def median_us(eng, rounds):
    eng.run(10)
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        eng.run(rounds)
        times.append(1e6 * (time.perf_counter() - t0) / rounds)
    return sorted(times)[1]


def dba_rows(a):
    from pydcop_amd.dba import DbaEngine
    g = G.random_coloring(100_000, seed=0, variant="hard", unary_noise=0, names=False)
    n = a.dba_rounds
    rows = {}
    eng = DbaEngine(g, Params(), infinity=1000, max_distance=4 * n + 100, seed=1, lib_path=a.lib)
    rows["dba"] = median_us(eng, n)
    assert not eng.finished
    extra = {"mask_bytes": eng.mask_bytes, "violations": eng.eval_cost(infinity=1000)[1]}
    eng.close()
    eng = GdbaEngine(g, Params(), modifier="A", violation="NZ", increase_mode="T", seed=1, lib_path=a.lib)
    rows["gdba"] = median_us(eng, n)
    eng.close()
    eng = MgmEngine(g, Params(), lib_path=a.lib)
    rows["mgm"] = median_us(eng, n)
    eng.close()
    for algo, us in rows.items():
        row = {"algo": algo, "instance": "coloring_100k_hard", "dtype": "int32" if algo == "dba" else "f64",
               "timing": "median3", "n_vars": g.n_vars, "us_per_cycle": round(us, 2)}
        if algo == "dba":
            row.update(extra, kernels="dba", ratio_to_gdba_T=round(us / rows["gdba"], 3), ratio_to_mgm=round(us / rows["mgm"], 3))
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=500)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--instances", nargs="*", default=["coloring_100k", "meeting_50k"])
    ap.add_argument("--kernels", nargs="*", default=["packed", "strided", "slots", "csr_walk"])
    ap.add_argument("--mgm2-rounds", type=int, default=200, help="0: no MGM-2 rows")
    ap.add_argument("--gdba-rounds", type=int, default=200, help="0: no GDBA rows")
    ap.add_argument("--dba-rounds", type=int, default=0, help="> 0: only the DBA / GDBA-T / MGM rows on the hard colouring")
    a = ap.parse_args()
    if a.dba_rounds > 0:
        return dba_rows(a)
    instances = [("coloring_100k", lambda: G.random_coloring(100_000, seed=0, names=False), Params()),
                 ("meeting_50k", lambda: G.meeting_like(50_000, dom=24, seed=0, names=False), Params(mode="max"))]
    for inst, g, p in instances:
        if inst not in a.instances:
            continue
        g = g()
        for kernels in a.kernels:
            os.environ["MAXSUM_LOCAL_SEARCH_GENERIC"] = {"packed": "0", "strided": "0", "slots": "2", "csr_walk": "1"}[kernels]
            os.environ.pop("MAXSUM_LOCAL_SEARCH_ROWS", None)
            if kernels == "strided":
                os.environ["MAXSUM_LOCAL_SEARCH_ROWS"] = "0"
            for name, make in (("dsa_B", lambda: DsaEngine(g, p, variant="B", seed=1, lib_path=a.lib)),
                               ("mgm", lambda: MgmEngine(g, p, lib_path=a.lib))):
                t0 = time.perf_counter()
                eng = make()
                setup_s = time.perf_counter() - t0
                eng.run(20)
                t0 = time.perf_counter()
                eng.run(a.cycles)
                dt = time.perf_counter() - t0
                print(json.dumps({"algo": name, "instance": inst, "kernels": kernels, "n_vars": g.n_vars,
                                  "cycles_per_s": round(a.cycles / dt, 1), "us_per_cycle": round(1e6 * dt / a.cycles, 2),
                                  "cost": eng.eval_cost()[0], "engine_setup_s": round(setup_s, 2)}), flush=True)
                eng.close()
        os.environ.pop("MAXSUM_LOCAL_SEARCH_GENERIC", None)
        os.environ.pop("MAXSUM_LOCAL_SEARCH_ROWS", None)
        for dtype in ("f64", "f32") if a.mgm2_rounds > 0 else ():
            t0 = time.perf_counter()
            eng = Mgm2Engine(g, Params(mode=p.mode, dtype=dtype), seed=1, lib_path=a.lib)
            setup_s = time.perf_counter() - t0
            eng.run(5)
            t0 = time.perf_counter()
            eng.run(a.mgm2_rounds)
            dt = time.perf_counter() - t0
            print(json.dumps({"algo": "mgm2", "instance": inst, "kernels": "mgm2", "dtype": dtype, "n_vars": g.n_vars,
                              "cycles_per_s": round(a.mgm2_rounds / dt, 1),
                              "us_per_cycle": round(1e6 * dt / a.mgm2_rounds, 2),
                              "cost": eng.eval_cost()[0], "engine_setup_s": round(setup_s, 2)}), flush=True)
            eng.close()
        for dtype in ("f64", "f32") if a.gdba_rounds > 0 else ():
            pd = Params(mode=p.mode, dtype=dtype)
            word = 8 if dtype == "f64" else 4

            def median_us(eng):
                eng.run(10)
                times = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    eng.run(a.gdba_rounds)
                    times.append(1e6 * (time.perf_counter() - t0) / a.gdba_rounds)
                return sorted(times)[1]

            eng = MgmEngine(g, pd, lib_path=a.lib)
            mgm_us = median_us(eng)
            eng.close()
            print(json.dumps({"algo": "mgm", "instance": inst, "kernels": "packed", "dtype": dtype, "timing": "median3",
                              "n_vars": g.n_vars, "us_per_cycle": round(mgm_us, 2)}), flush=True)
            for mode in ("E", "C"):
                t0 = time.perf_counter()
                eng = GdbaEngine(g, pd, modifier="A", violation="NZ" if p.mode == "min" else "NM", increase_mode=mode,
                                 seed=1, lib_path=a.lib)
                setup_s = time.perf_counter() - t0
                us = median_us(eng)
                # what a round can touch: the tables, the modifier pool, the slot view, the per-variable state
                resident = (g.tables.shape[0] * word + eng.pool_bytes + len(g.var_edges) * (8 + 4 + 4 + 8 + word + 1)
                            + (g.n_edges - len(g.var_edges) + g.n_edges) * 8 + g.n_vars * (4 + word + 1 + 8 + word))
                print(json.dumps({"algo": "gdba", "instance": inst, "kernels": "gdba", "dtype": dtype, "timing": "median3", "increase_mode": mode,
                                  "n_vars": g.n_vars, "us_per_cycle": round(us, 2), "ratio_to_mgm": round(us / mgm_us, 2),
                                  "pool_bytes": eng.pool_bytes, "resident_bytes": int(resident),
                                  "resident_gb_per_s": round(resident / us / 1e3, 1),
                                  "cost": eng.eval_cost()[0], "engine_setup_s": round(setup_s, 2)}), flush=True)
                eng.close()


if __name__ == "__main__":
    main()
