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
`--replicas R [R ...]` prints the rows of the DSA replica engine instead (DsaEngine(replicas=R), dsa.hip): on
`random_coloring` at `--replica-sizes` variables (f64, variant B), the time of a cycle of ALL replicas against R times
the time of a cycle of a single-seed engine (what R restarts cost one engine after the other), the two sides
alternated in one process, windows of `--window` seconds after a warm-up of `--warmup` seconds per engine,
`--repeats` pairs (the rows give every repeat: the spread); then the same engine with `best_every` 1 and 10, and the
device cost reduction (`replica_costs`) against R host `eval_cost` calls with their copies back.  The single-seed side
is this library's engine ("baseline": "this") or, with `--baseline-lib PATH`, the `mxs_dsa_create` of another build
of the library -- e.g. the parent commit's, built from `git archive <commit> pydcop_amd/csrc include` with the
csrc Makefile -- loaded beside this one ("baseline": its mxs_version).
`--replica-algos` (default: dsa mgm) chooses whose rows are printed.  The MGM rows ("algo": "mgm", MgmEngine(draws="keyed",
replicas=R), mgm.hip) follow the same protocol, the single side being the fixed-draw engine (`mxs_mgm_create` of this
library or of `--baseline-lib`: a keyed single run costs the same per round); before them, per size, two rows without
replicas: "fixed_vs_baseline" (this library's fixed-draw engine against the single side: the same kernel
instantiations) and "keyed_vs_fixed" (the keyed one-replica engine against the fixed-draw one: what the draw code
costs; MGM reaches its fixed point after a few rounds, where draw 11 is no longer made, so the row also times the
first 12 rounds after reset(), "fresh_us_per_round").  The MGM-2 rows (`--replica-algos mgm2`; "algo": "mgm2",
Mgm2Engine(replicas=R), mgm2.h) follow the protocol of the MGM rows: the single side is `mxs_mgm2_create` of this
library or of `--baseline-lib`; per size first "instance_to_instance" (two engines of the single side against each
other: the spread of the protocol itself) and "single_vs_baseline" (this library's `mxs_mgm2_create` against the single
side), then one "replicas" row per R.  The GDBA rows (`--replica-algos gdba`; "algo": "gdba_A_NZ_<mode>",
GdbaEngine(replicas=R), gdba.h, increase modes `--gdba-modes`) follow the protocol of the MGM-2 rows with `mxs_gdba_create`
as the single side; every timed window starts from reset() and is capped at 20 000 rounds (the counters allow 65535),
and a row also has the rounds with the best state tracked every round and every 10th ("best_every_1_us_per_round",
"best_every_10_us_per_round").  The DBA rows (`--replica-algos dba`; "algo": "dba", DbaEngine(replicas=R), dba.h)
follow the protocol of the MGM-2 rows with `mxs_dba_create` as the single side, on the HARD colouring (`infinity: 1000`,
no unary noise) with a `max_distance` no counter reaches, so that nothing stops; a "replicas" row gives R times the single
run's time beside the time of a round of all replicas ("R_singles_us_per_round") and the time of the device's violation
count ("replica_violations_us": mxs_dba_replica_violations with its copy back).
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


class BaselineDsa:
    """The single-seed DSA engine of ANOTHER build of the library (--baseline-lib), through the entry points every
    version has: mxs_dsa_create / _run / _destroy.  Loaded with plain ctypes beside the library under test."""

    def __init__(self, path, g, p, seed):
        import ctypes as C
        from pydcop_amd.engine import load_library
        load_library()                       # (the HIP runtime first: the libraries are linked without it)
        self._lib = C.CDLL(os.path.abspath(path))
        self._lib.mxs_version.restype = C.c_int32
        self.version = int(self._lib.mxs_version())
        self._lib.mxs_dsa_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_uint64,
                                             C.c_int32, C.c_void_p]
        self._lib.mxs_dsa_run.argtypes = [C.c_void_p, C.c_int32]
        self._lib.mxs_dsa_destroy.argtypes = [C.c_void_p]
        self._g, self._p = g.to_c(), p.to_c()      # (kept alive)
        self._h = C.c_void_p()
        rc = self._lib.mxs_dsa_create(C.byref(self._g), C.byref(self._p), 1, 0.7, 0, seed, 0, C.byref(self._h))
        if rc:
            raise RuntimeError(f"mxs_dsa_create of {path}: {rc}")

    def run(self, n):
        if self._lib.mxs_dsa_run(self._h, int(n)):
            raise RuntimeError("mxs_dsa_run of the baseline library failed")

    def close(self):
        self._lib.mxs_dsa_destroy(self._h)


class BaselineMgm:
    """The fixed-draw MGM engine of ANOTHER build of the library (--baseline-lib): mxs_mgm_create / _run / _destroy."""

    def __init__(self, path, g, p):
        import ctypes as C
        from pydcop_amd.engine import load_library
        load_library()                       # (the HIP runtime first: the libraries are linked without it)
        self._lib = C.CDLL(os.path.abspath(path))
        self._lib.mxs_version.restype = C.c_int32
        self.version = int(self._lib.mxs_version())
        self._lib.mxs_mgm_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        self._lib.mxs_mgm_run.argtypes = [C.c_void_p, C.c_int32]
        self._lib.mxs_mgm_destroy.argtypes = [C.c_void_p]
        self._g, self._p = g.to_c(), p.to_c()      # (kept alive)
        self._h = C.c_void_p()
        rc = self._lib.mxs_mgm_create(C.byref(self._g), C.byref(self._p), None, 0, C.byref(self._h))
        if rc:
            raise RuntimeError(f"mxs_mgm_create of {path}: {rc}")

    def run(self, n):
        if self._lib.mxs_mgm_run(self._h, int(n)):
            raise RuntimeError("mxs_mgm_run of the baseline library failed")

    def close(self):
        self._lib.mxs_mgm_destroy(self._h)


class BaselineMgm2:
    """The MGM-2 engine of ANOTHER build of the library (--baseline-lib): mxs_mgm2_create / _run / _destroy."""

    def __init__(self, path, g, p, seed):
        import ctypes as C
        from pydcop_amd.engine import load_library
        load_library()                       # (the HIP runtime first: the libraries are linked without it)
        self._lib = C.CDLL(os.path.abspath(path))
        self._lib.mxs_version.restype = C.c_int32
        self.version = int(self._lib.mxs_version())
        self._lib.mxs_mgm2_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_uint64,
                                              C.c_int32, C.c_void_p]
        self._lib.mxs_mgm2_run.argtypes = [C.c_void_p, C.c_int32]
        self._lib.mxs_mgm2_destroy.argtypes = [C.c_void_p]
        self._g, self._p = g.to_c(), p.to_c()      # (kept alive)
        self._h = C.c_void_p()
        rc = self._lib.mxs_mgm2_create(C.byref(self._g), C.byref(self._p), None, 0.5, 0, seed, 0, C.byref(self._h))
        if rc:
            raise RuntimeError(f"mxs_mgm2_create of {path}: {rc}")

    def run(self, n):
        if self._lib.mxs_mgm2_run(self._h, int(n)):
            raise RuntimeError("mxs_mgm2_run of the baseline library failed")

    def close(self):
        self._lib.mxs_mgm2_destroy(self._h)


def timed_us(eng, cycles):
    t0 = time.perf_counter()
    eng.run(cycles)
    return 1e6 * (time.perf_counter() - t0) / cycles


def cycles_for(eng, window_s, warmup_s=0.0):
    """the number of cycles that fill the window, after a warm-up of `warmup_s` seconds"""
    eng.run(20)
    us = timed_us(eng, 50)
    if warmup_s > 0:
        us = timed_us(eng, max(50, int(warmup_s * 1e6 / max(us, 1e-3))))
    return max(50, int(window_s * 1e6 / max(us, 1e-3)))


def replica_rows(a):
    for n_vars in a.replica_sizes:
        g = G.random_coloring(n_vars, seed=0, names=False)
        p = Params()
        for R in a.replicas:
            # both engines are created and warmed up anew for every row: neither side carries the history of the
            # rows before it into the ratio
            if a.baseline_lib:
                single = BaselineDsa(a.baseline_lib, g, p, 1)
                baseline = f"mxs_version {single.version}"
            else:
                single, baseline = DsaEngine(g, p, variant="B", seed=1, lib_path=a.lib), "this"
            n_single = cycles_for(single, a.window, a.warmup)
            eng = DsaEngine(g, p, variant="B", seed=1, replicas=R, lib_path=a.lib)
            n_rep = cycles_for(eng, a.window, a.warmup)
            one, many = [], []
            for _ in range(a.repeats):      # alternated: both sides see the same machine
                one.append(timed_us(single, n_single))
                many.append(timed_us(eng, n_rep))
            row = {"algo": "dsa_B", "instance": f"coloring_{n_vars}", "dtype": "f64", "n_vars": n_vars, "replicas": R,
                   "baseline": baseline, "single_us_per_cycle": [round(x, 2) for x in one], "replicas_us_per_cycle": [round(x, 2) for x in many],
                   "ratio_R_singles_to_replicas": round(R * sorted(one)[len(one) // 2] / sorted(many)[len(many) // 2], 2)}
            for every in (1, 10):
                eng.track_best(every, float("inf"))
                eng.run(20)
                row[f"best_every_{every}_us_per_cycle"] = [round(timed_us(eng, n_rep), 2) for _ in range(a.repeats)]
            eng.track_best(0, float("inf"))
            reps = max(3, int(0.2 * a.window * 1e6 / max(many[0], 1.0)))
            t0 = time.perf_counter()
            for _ in range(reps):
                dev = eng.replica_costs()
            row["replica_costs_us"] = round(1e6 * (time.perf_counter() - t0) / reps, 1)
            reps = max(1, min(reps, 2000 // R))
            t0 = time.perf_counter()
            for _ in range(reps):
                host = [eng.eval_cost(eng.assignment(r)[0]) for r in range(R)]
            row["host_eval_cost_us"] = round(1e6 * (time.perf_counter() - t0) / reps, 1)
            assert all(abs(dev[0][r] - host[r][0]) <= 1e-9 * max(1.0, abs(host[r][0])) for r in range(R))
            print(json.dumps(row), flush=True)
            eng.close()
            single.close()


def alternated(a, left, right):
    """both engines warmed up, then `repeats` alternated windows: (us per round of left, of right)"""
    n_left, n_right = cycles_for(left, a.window, a.warmup), cycles_for(right, a.window, a.warmup)
    one, other = [], []
    for _ in range(a.repeats):
        one.append(round(timed_us(left, n_left), 2))
        other.append(round(timed_us(right, n_right), 2))
    return one, other


def median(xs):
    return sorted(xs)[len(xs) // 2]


def mgm_replica_rows(a):
    for n_vars in a.replica_sizes:
        g = G.random_coloring(n_vars, seed=0, names=False)
        p = Params()

        def single_side():
            if a.baseline_lib:
                e = BaselineMgm(a.baseline_lib, g, p)
                return e, f"mxs_version {e.version}"
            return MgmEngine(g, p, lib_path=a.lib), "this"

        base = {"algo": "mgm", "instance": f"coloring_{n_vars}", "dtype": "f64", "n_vars": n_vars}
        # the fixed-draw engine of this library against the single side
        single, baseline = single_side()
        fixed = MgmEngine(g, p, lib_path=a.lib)
        one, mine = alternated(a, single, fixed)
        print(json.dumps(dict(base, row="fixed_vs_baseline", baseline=baseline, single_us_per_round=one,
                              fixed_us_per_round=mine, ratio_fixed_to_single=round(median(mine) / median(one), 4))), flush=True)
        single.close()
        # the keyed one-replica engine against the fixed-draw one
        keyed = MgmEngine(g, p, draws="keyed", seed=1, lib_path=a.lib)
        f_us, k_us = alternated(a, fixed, keyed)
        fresh = {}
        for name, eng in (("fixed", fixed), ("keyed", keyed)):
            ts = []
            for _ in range(a.repeats):
                total = 0.0
                for _ in range(40):
                    eng.reset()
                    t0 = time.perf_counter()
                    eng.run(12)
                    total += time.perf_counter() - t0
                ts.append(round(1e6 * total / (40 * 12), 2))
            fresh[name] = ts
        print(json.dumps(dict(base, row="keyed_vs_fixed", fixed_us_per_round=f_us, keyed_us_per_round=k_us,
                              ratio_keyed_to_fixed=round(median(k_us) / median(f_us), 4),
                              fresh_us_per_round=fresh)), flush=True)
        fixed.close(), keyed.close()
        for R in a.replicas:
            single, baseline = single_side()
            eng = MgmEngine(g, p, draws="keyed", seed=1, replicas=R, lib_path=a.lib)
            one, many = alternated(a, single, eng)
            row = dict(base, row="replicas", replicas=R, baseline=baseline, single_us_per_round=one,
                       replicas_us_per_round=many, ratio_R_singles_to_replicas=round(R * median(one) / median(many), 2))
            reps = max(3, int(0.2 * a.window * 1e6 / max(many[0], 1.0)))
            t0 = time.perf_counter()
            for _ in range(reps):
                dev = eng.replica_costs()
            row["replica_costs_us"] = round(1e6 * (time.perf_counter() - t0) / reps, 1)
            reps = max(1, min(reps, 2000 // R))
            t0 = time.perf_counter()
            for _ in range(reps):
                host = [eng.eval_cost(eng.assignment(r)[0]) for r in range(R)]
            row["host_eval_cost_us"] = round(1e6 * (time.perf_counter() - t0) / reps, 1)
            assert all(abs(dev[0][r] - host[r][0]) <= 1e-9 * max(1.0, abs(host[r][0])) for r in range(R))
            print(json.dumps(row), flush=True)
            eng.close()
            single.close()


def mgm2_replica_rows(a):
    for n_vars in a.replica_sizes:
        g = G.random_coloring(n_vars, seed=0, names=False)
        p = Params()

        def single_side():
            if a.baseline_lib:
                e = BaselineMgm2(a.baseline_lib, g, p, 1)
                return e, f"mxs_version {e.version}"
            return Mgm2Engine(g, p, seed=1, lib_path=a.lib), "this"

        base = {"algo": "mgm2", "instance": f"coloring_{n_vars}", "dtype": "f64", "n_vars": n_vars}
        # two engines of the single side against each other: what the protocol itself spreads
        left, baseline = single_side()
        right, _ = single_side()
        one, other = alternated(a, left, right)
        print(json.dumps(dict(base, row="instance_to_instance", baseline=baseline, left_us_per_round=one,
                              right_us_per_round=other, ratio_right_to_left=round(median(other) / median(one), 4))),
              flush=True)
        right.close()
        # this library's mxs_mgm2_create against the single side
        mine = Mgm2Engine(g, p, seed=1, lib_path=a.lib)
        one, new = alternated(a, left, mine)
        print(json.dumps(dict(base, row="single_vs_baseline", baseline=baseline, single_us_per_round=one,
                              this_us_per_round=new, ratio_this_to_single=round(median(new) / median(one), 4))), flush=True)
        left.close(), mine.close()
        for R in a.replicas:
            single, baseline = single_side()
            eng = Mgm2Engine(g, p, seed=1, replicas=R, lib_path=a.lib) if R > 1 else \
                Mgm2Engine(g, p, seeds=[1], replicas=1, lib_path=a.lib)       # (R = 1 through the replica kernels too)
            one, many = alternated(a, single, eng)
            row = dict(base, row="replicas", replicas=R, baseline=baseline, single_us_per_round=one,
                       replicas_us_per_round=many, ratio_R_singles_to_replicas=round(R * median(one) / median(many), 2))
            reps = max(3, int(0.2 * a.window * 1e6 / max(many[0], 1.0)))
            t0 = time.perf_counter()
            for _ in range(reps):
                dev = eng.replica_costs()
            row["replica_costs_us"] = round(1e6 * (time.perf_counter() - t0) / reps, 1)
            reps = max(1, min(reps, 2000 // R))
            t0 = time.perf_counter()
            for _ in range(reps):
                host = [eng.eval_cost(eng.assignment(r)[0]) for r in range(R)]
            row["host_eval_cost_us"] = round(1e6 * (time.perf_counter() - t0) / reps, 1)
            assert all(abs(dev[0][r] - host[r][0]) <= 1e-9 * max(1.0, abs(host[r][0])) for r in range(R))
            print(json.dumps(row), flush=True)
            eng.close()
            single.close()


class BaselineGdba:
    """The GDBA engine of ANOTHER build of the library (--baseline-lib): mxs_gdba_create / _reset / _run / _destroy."""

    def __init__(self, path, g, p, seed, codes):
        import ctypes as C
        from pydcop_amd.engine import load_library
        load_library()                       # (the HIP runtime first: the libraries are linked without it)
        self._lib = C.CDLL(os.path.abspath(path))
        self._lib.mxs_version.restype = C.c_int32
        self.version = int(self._lib.mxs_version())
        self._lib.mxs_gdba_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                              C.c_uint64, C.c_int64, C.c_int32, C.c_void_p]
        self._lib.mxs_gdba_run.argtypes = [C.c_void_p, C.c_int32]
        self._lib.mxs_gdba_reset.argtypes = [C.c_void_p]
        self._lib.mxs_gdba_destroy.argtypes = [C.c_void_p]
        self._g, self._p = g.to_c(), p.to_c()      # (kept alive)
        self._h = C.c_void_p()
        rc = self._lib.mxs_gdba_create(C.byref(self._g), C.byref(self._p), None, None, codes[0], codes[1], codes[2], seed, 0,
                                       0, C.byref(self._h))
        if rc:
            raise RuntimeError(f"mxs_gdba_create of {path}: {rc}")

    def run(self, n):
        if self._lib.mxs_gdba_run(self._h, int(n)):
            raise RuntimeError("mxs_gdba_run of the baseline library failed")

    def reset(self):
        if self._lib.mxs_gdba_reset(self._h):
            raise RuntimeError("mxs_gdba_reset of the baseline library failed")

    def close(self):
        self._lib.mxs_gdba_destroy(self._h)


GDBA_WINDOW_ROUNDS = 20_000      # (the counters are 16 bits wide: a window starts from reset() and stays below 65535)


def gdba_rounds_for(eng, window_s):
    """the number of rounds that fill the window, at most GDBA_WINDOW_ROUNDS; warms the engine up on the way"""
    eng.reset()
    eng.run(20)
    us = timed_us(eng, 200)
    return max(50, min(GDBA_WINDOW_ROUNDS, int(window_s * 1e6 / max(us, 1e-3))))


def gdba_timed_us(eng, rounds):
    eng.reset()
    eng.run(20)
    return round(timed_us(eng, rounds), 2)


def gdba_alternated(a, left, right):
    n_left, n_right = gdba_rounds_for(left, a.window), gdba_rounds_for(right, a.window)
    one, other = [], []
    for _ in range(a.repeats):
        one.append(gdba_timed_us(left, n_left))
        other.append(gdba_timed_us(right, n_right))
    return one, other


def gdba_replica_rows(a):
    """The protocol of the MGM-2 rows for GdbaEngine(replicas=R) (gdba.h), modifier A / violation NZ, increase modes T
    and C: every timed window starts from reset() plus 20 rounds (the counters allow 65535 rounds) and is capped at
    GDBA_WINDOW_ROUNDS rounds.  Columns beside the MGM-2 ones: the rounds with track_best(1) and track_best(10)."""
    from pydcop_amd.gdba import GdbaEngine, check_params
    for inc in a.gdba_modes:
        kw = dict(modifier="A", violation="NZ", increase_mode=inc)
        codes = check_params("A", "NZ", inc)
        for n_vars in a.replica_sizes:
            g = G.random_coloring(n_vars, seed=0, names=False)
            p = Params()

            def single_side():
                if a.baseline_lib:
                    e = BaselineGdba(a.baseline_lib, g, p, 1, codes)
                    return e, f"mxs_version {e.version}"
                return GdbaEngine(g, p, seed=1, lib_path=a.lib, **kw), "this"

            base = {"algo": f"gdba_A_NZ_{inc}", "instance": f"coloring_{n_vars}", "dtype": "f64", "n_vars": n_vars}
            # two engines of the single side against each other: what the protocol itself spreads
            left, baseline = single_side()
            right, _ = single_side()
            one, other = gdba_alternated(a, left, right)
            print(json.dumps(dict(base, row="instance_to_instance", baseline=baseline, left_us_per_round=one,
                                  right_us_per_round=other, ratio_right_to_left=round(median(other) / median(one), 4))),
                  flush=True)
            right.close()
            # this library's mxs_gdba_create against the single side
            mine = GdbaEngine(g, p, seed=1, lib_path=a.lib, **kw)
            one, new = gdba_alternated(a, left, mine)
            print(json.dumps(dict(base, row="single_vs_baseline", baseline=baseline, single_us_per_round=one,
                                  this_us_per_round=new, ratio_this_to_single=round(median(new) / median(one), 4))), flush=True)
            left.close(), mine.close()
            for R in a.replicas:
                single, baseline = single_side()
                eng = GdbaEngine(g, p, seeds=[1 + r for r in range(R)], replicas=R, lib_path=a.lib, **kw)   # (R = 1 too)
                n_single, n_rep = gdba_rounds_for(single, a.window), gdba_rounds_for(eng, a.window)
                one, many = [], []
                for _ in range(a.repeats):
                    one.append(gdba_timed_us(single, n_single))
                    many.append(gdba_timed_us(eng, n_rep))
                row = dict(base, row="replicas", replicas=R, baseline=baseline, single_us_per_round=one,
                           replicas_us_per_round=many, ratio_R_singles_to_replicas=round(R * median(one) / median(many), 2))
                for every in (1, 10):
                    eng.track_best(every, float("inf"))
                    row[f"best_every_{every}_us_per_round"] = [gdba_timed_us(eng, n_rep) for _ in range(a.repeats)]
                eng.track_best(0, float("inf"))
                reps = max(3, min(2000, int(0.2 * a.window * 1e6 / max(many[0], 1.0))))
                t0 = time.perf_counter()
                for _ in range(reps):
                    dev = eng.replica_costs()
                row["replica_costs_us"] = round(1e6 * (time.perf_counter() - t0) / reps, 1)
                reps = max(1, min(reps, 2000 // R))
                t0 = time.perf_counter()
                for _ in range(reps):
                    host = [eng.eval_cost(eng.assignment(r)[0]) for r in range(R)]
                row["host_eval_cost_us"] = round(1e6 * (time.perf_counter() - t0) / reps, 1)
                assert all(abs(dev[0][r] - host[r][0]) <= 1e-9 * max(1.0, abs(host[r][0])) for r in range(R))
                print(json.dumps(row), flush=True)
                eng.close()
                single.close()


class BaselineDba:
    """The DBA engine of ANOTHER build of the library (--baseline-lib): mxs_dba_create / _run / _destroy."""

    def __init__(self, path, g, p, seed, infinity, max_distance):
        import ctypes as C
        from pydcop_amd.engine import load_library
        load_library()                       # (the HIP runtime first: the libraries are linked without it)
        self._lib = C.CDLL(os.path.abspath(path))
        self._lib.mxs_version.restype = C.c_int32
        self.version = int(self._lib.mxs_version())
        self._lib.mxs_dba_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_uint64,
                                             C.c_int64, C.c_int32, C.c_void_p]
        self._lib.mxs_dba_run.argtypes = [C.c_void_p, C.c_int32]
        self._lib.mxs_dba_destroy.argtypes = [C.c_void_p]
        self._g, self._p = g.to_c(), p.to_c()      # (kept alive)
        self._h = C.c_void_p()
        rc = self._lib.mxs_dba_create(C.byref(self._g), C.byref(self._p), None, float(infinity), int(max_distance), seed, 0,
                                      0, C.byref(self._h))
        if rc:
            raise RuntimeError(f"mxs_dba_create of {path}: {rc}")

    def run(self, n):
        if self._lib.mxs_dba_run(self._h, int(n)):
            raise RuntimeError("mxs_dba_run of the baseline library failed")

    def close(self):
        self._lib.mxs_dba_destroy(self._h)


DBA_NEVER = 2 ** 31 - 1          # a max_distance no termination counter reaches: nothing stops in a window


def dba_replica_rows(a):
    """The protocol of the MGM-2 rows for DbaEngine(replicas=R) (dba.h) on the HARD colouring (`infinity: 1000`, no
    unary noise), `max_distance` above any round count so that nothing stops.  A "replicas" row also has the time of
    the device's violation count (`violations()`: mxs_dba_replica_violations, its copy back included)."""
    from pydcop_amd.dba import DbaEngine
    kw = dict(infinity=1000, max_distance=DBA_NEVER)
    for n_vars in a.replica_sizes:
        g = G.random_coloring(n_vars, seed=0, variant="hard", unary_noise=0, names=False)
        p = Params()

        def single_side():
            if a.baseline_lib:
                e = BaselineDba(a.baseline_lib, g, p, 1, kw["infinity"], kw["max_distance"])
                return e, f"mxs_version {e.version}"
            return DbaEngine(g, p, seed=1, lib_path=a.lib, **kw), "this"

        base = {"algo": "dba", "instance": f"coloring_hard_{n_vars}", "dtype": "int32", "n_vars": n_vars}
        # two engines of the single side against each other: what the protocol itself spreads
        left, baseline = single_side()
        right, _ = single_side()
        one, other = alternated(a, left, right)
        print(json.dumps(dict(base, row="instance_to_instance", baseline=baseline, left_us_per_round=one,
                              right_us_per_round=other, ratio_right_to_left=round(median(other) / median(one), 4))),
              flush=True)
        right.close()
        # this library's mxs_dba_create against the single side
        mine = DbaEngine(g, p, seed=1, lib_path=a.lib, **kw)
        one, new = alternated(a, left, mine)
        print(json.dumps(dict(base, row="single_vs_baseline", baseline=baseline, single_us_per_round=one,
                              this_us_per_round=new, ratio_this_to_single=round(median(new) / median(one), 4))), flush=True)
        left.close(), mine.close()
        for R in a.replicas:
            single, baseline = single_side()
            eng = DbaEngine(g, p, seeds=[1 + r for r in range(R)], replicas=R, lib_path=a.lib, **kw)   # (R = 1 too)
            one, many = alternated(a, single, eng)
            assert not eng.finished
            row = dict(base, row="replicas", replicas=R, baseline=baseline, single_us_per_round=one,
                       replicas_us_per_round=many, R_singles_us_per_round=round(R * median(one), 2),
                       ratio_R_singles_to_replicas=round(R * median(one) / median(many), 2))
            reps = max(3, min(2000, int(0.2 * a.window * 1e6 / max(many[0], 1.0))))
            t0 = time.perf_counter()
            for _ in range(reps):
                viol = eng.violations()
            row["replica_violations_us"] = round(1e6 * (time.perf_counter() - t0) / reps, 1)
            row["violations"] = [int(v) for v in viol[:8]]
            print(json.dumps(row), flush=True)
            eng.close()
            single.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=500)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--instances", nargs="*", default=["coloring_100k", "meeting_50k"])
    ap.add_argument("--kernels", nargs="*", default=["packed", "strided", "slots", "csr_walk"])
    ap.add_argument("--mgm2-rounds", type=int, default=200, help="0: no MGM-2 rows")
    ap.add_argument("--gdba-rounds", type=int, default=200, help="0: no GDBA rows")
    ap.add_argument("--dba-rounds", type=int, default=0, help="> 0: only the DBA / GDBA-T / MGM rows on the hard colouring")
    ap.add_argument("--replicas", type=int, nargs="*", default=[], help="the replica rows only (DSA, MGM, MGM-2): R values")
    ap.add_argument("--replica-sizes", type=int, nargs="*", default=[1000, 10_000, 100_000])
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window of the replica rows")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=float, default=0.5, help="seconds of warm-up per engine of the replica rows")
    ap.add_argument("--baseline-lib", default=None,
                    help="replica rows: the single-seed side from this other build of the library (mxs_dsa_create)")
    ap.add_argument("--replica-algos", nargs="*", default=["dsa", "mgm"], choices=["dsa", "mgm", "mgm2", "gdba", "dba"])
    ap.add_argument("--gdba-modes", nargs="*", default=["T", "C"], choices=["E", "R", "C", "T"],
                    help="the increase modes of the GDBA replica rows")
    a = ap.parse_args()
    if a.replicas:
        if "dsa" in a.replica_algos:
            replica_rows(a)
        if "mgm" in a.replica_algos:
            mgm_replica_rows(a)
        if "mgm2" in a.replica_algos:
            mgm2_replica_rows(a)
        if "gdba" in a.replica_algos:
            gdba_replica_rows(a)
        if "dba" in a.replica_algos:
            dba_replica_rows(a)
        return
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
