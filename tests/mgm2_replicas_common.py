"""MGM-2 replicas (Mgm2Engine(replicas=R): R seeded runs in one engine, pydcop_amd/csrc/mgm2.h) against
tests/mgm2_oracle.py: replica r is bit for bit OracleMgm2(seed=seeds[r]); the device cost against eval_cost; the best
replica against the winner derived from the oracle alone; the fixtures recorded from the reference (tests/golden/mgm2).
The test functions live here, below the helpers; tests/test_mgm2_replicas_emu.py (emulated build) and
tests/test_gpu_mgm2_replicas.py (the HIP library) import them and provide the `lib_path` fixture, so the two runs
cannot drift apart."""
import ctypes as C
import os

import numpy as np
import pytest

from dsa_replicas_common import check_costs, winner
from mgm2_common import check_golden, load_mgm2_golden, mgm2_golden_files
from mgm2_oracle import OracleMgm2
from mgm_common import shuffled_names, with_init
from pydcop_amd import generators as G
from pydcop_amd.engine import MaxSumGpuError, load_library
from pydcop_amd.graph import Params
from pydcop_amd.mgm2 import Mgm2Engine

KEYS = ("idx", "has_cost", "cost")
HARD = "hard150_coordinated"
MXS_E_INVALID = -1


def parity_cases():
    """(id, instance, Params kwargs, MGM-2 kwargs, R): the smallest shapes that cross each boundary"""
    return [
        # 3 variable blocks and 6 offer blocks per replica, both last blocks partial; name-rank ties
        (HARD, lambda: shuffled_names(G.random_coloring(150, seed=63, variant="hard"), 63), {},
         dict(favor="coordinated"), 3),
        ("f32_max_no", lambda: G.random_coloring(70, seed=33), {"mode": "max", "dtype": "f32"}, dict(favor="no"), 2),
        ("isolated_max", lambda: G.random_coloring(60, avg_degree=1, seed=36), {"mode": "max"}, {}, 5),
        ("unequal_domains_arity3", lambda: G.random_mixed(40, 70, seed=65), {}, {}, 3),
        ("with_init", lambda: with_init(G.random_coloring(45, seed=37, variant="hard"), 37), {}, {}, 2),
        ("meeting_d6_max", lambda: G.meeting_like(20, dom=6, seed=72), {"mode": "max"}, dict(threshold=0.7), 3),
        ("threshold_0", lambda: G.random_coloring(45, seed=70), {}, dict(threshold=0.0), 2),
        ("threshold_1", lambda: G.random_coloring(45, seed=71), {}, dict(threshold=1.0), 2),
    ]


def same_state(eng, oras, what):
    for r, ora in oras.items():
        se, so = eng.state(r), ora.state()
        for k in KEYS:
            np.testing.assert_array_equal(se[k], so[k], err_msg=f"{k} of replica {r} {what}")


def compare_replicas(graph, params, kw, replicas, lib_path=None, seed=5, seeds=None, check=None, steps=(0, 1, 1, 3, 10)):
    """every replica of `check` (default: all) against OracleMgm2(seed=seeds[r]): idx, has_cost and cost bit for bit
    after 0, 1, 2, 5 and 15 rounds, then after reset() and 4 rounds.  Returns the engine (after those 4 rounds), the
    oracles' start states, their states after the steps and their pair moves during the steps."""
    eng = Mgm2Engine(graph, params, seed=seed, seeds=seeds, replicas=replicas, lib_path=lib_path, **kw)
    assert eng.replicas == replicas and len(eng.seeds) == replicas
    if seeds is None:
        assert eng.seeds == [seed + r for r in range(replicas)]
    check = list(range(replicas)) if check is None else list(check)
    oras = {r: OracleMgm2(graph, params, seed=eng.seeds[r], **kw) for r in check}
    done, starts = 0, None
    for n in steps:
        eng.run(n)
        done += n
        for ora in oras.values():
            ora.run(n)
            assert eng.cycle_count == ora.cycle_count == done
        same_state(eng, oras, f"after {done} rounds")
        check_costs(eng, check)
        if starts is None:
            starts = {r: o.state()["idx"] for r, o in oras.items()}
    finals = {r: o.state()["idx"] for r, o in oras.items()}
    pair_moves = {r: o.pair_moves for r, o in oras.items()}
    eng.reset()
    eng.run(4)
    for ora in oras.values():
        ora.reset(), ora.run(4)
        assert eng.cycle_count == ora.cycle_count == 4
    same_state(eng, oras, "after reset() and 4 rounds")
    # replica 0 is what the single-state calls mean
    np.testing.assert_array_equal(eng.assignment()[0], eng.assignment(0)[0])
    assert eng.eval_cost() == eng.eval_cost(eng.assignment(0)[0])
    return eng, starts, finals, pair_moves


def oracle_finals(g, params, kw, seeds, rounds, infinity):
    """per seed (violations, cost, idx) of the oracle's state after `rounds` rounds, by the oracle's own eval_cost"""
    out = []
    for s in seeds:
        o = OracleMgm2(g, params, seed=s, **kw)
        o.run(rounds)
        idx = o.state()["idx"]
        cost, viol = o.eval_cost(idx, infinity)
        out.append((viol, cost, idx))
    return out


# ---- the tests; `lib_path`: the fixture of the importing file (the emulated build, or None = the HIP library)

@pytest.mark.parametrize("case", parity_cases(), ids=lambda c: c[0])
def test_every_replica_equals_the_oracle(case, lib_path):
    name, make, pkw, kw, replicas = case
    eng, starts, finals, pair_moves = compare_replicas(make(), Params(**pkw), kw, replicas, lib_path=lib_path)
    eng.close()
    if name == HARD:
        # what keeps the comparison from passing with the replica fold left out (conditions on the oracle side):
        # committed pairs move in every run, the runs start apart and end apart
        assert all(m >= 1 for m in pair_moves.values()), pair_moves
        assert all((starts[r] != starts[0]).any() for r in starts if r)
        assert all((finals[r] != finals[0]).any() for r in finals if r)


def test_many_small_replicas(lib_path):
    """more blocks than one replica needs, and the highest offsets: 64 replicas of 12 variables"""
    eng, *_ = compare_replicas(G.random_coloring(12, seed=31, variant="hard"), Params(), {}, 64, lib_path=lib_path,
                               check=(0, 1, 31, 32, 63))
    eng.close()


def test_explicit_seeds(lib_path):
    seeds = [9, 9, 2 ** 64 - 1, 2 ** 63]
    eng, *_ = compare_replicas(G.random_coloring(45, seed=31, variant="hard"), Params(), dict(favor="no"), 4,
                               lib_path=lib_path, seeds=seeds)
    assert eng.seeds == seeds
    s0, s1 = eng.state(0), eng.state(1)
    for k in KEYS:                                                 # the same seed: the same run
        np.testing.assert_array_equal(s0[k], s1[k])
    eng.close()
    with Mgm2Engine(G.random_coloring(10, seed=1), seed=2 ** 64 - 1, replicas=2, lib_path=lib_path) as e:
        assert e.seeds == [2 ** 64 - 1, 0]                         # the default seeds wrap modulo 2**64


def test_one_replica_equals_the_single_run_engine(lib_path):
    """seeds=[s] goes through mxs_mgm2_create_replicas, seed=s through mxs_mgm2_create: the same run, the oracle's"""
    g, s = shuffled_names(G.random_coloring(80, seed=63, variant="hard"), 63), 11
    kw = dict(favor="coordinated", threshold=0.6)
    with Mgm2Engine(g, Params(), seeds=[s], replicas=1, lib_path=lib_path, **kw) as rep, \
            Mgm2Engine(g, Params(), seed=s, lib_path=lib_path, **kw) as one:
        n = C.c_int32(0)
        for e in (rep, one):
            e._call("replicas", C.byref(n))
            assert n.value == 1 and e.replicas == 1 and e.seeds == [s]
        ora = OracleMgm2(g, Params(), seed=s, **kw)
        for n_rounds in (0, 1, 6):
            rep.run(n_rounds), one.run(n_rounds), ora.run(n_rounds)
            for k in KEYS:
                np.testing.assert_array_equal(rep.state()[k], one.state()[k])
                np.testing.assert_array_equal(rep.state()[k], ora.state()[k])
        assert ora.pair_moves >= 1
        with pytest.raises(MaxSumGpuError, match="replica"):
            one.state(1)
        with pytest.raises(MaxSumGpuError, match="replica"):
            rep.state(1)


def test_refusals(lib_path):
    g = G.random_coloring(12, seed=1)
    for n in (0, 4097):
        with pytest.raises(MaxSumGpuError, match=f"error {MXS_E_INVALID}: .*replicas"):
            Mgm2Engine(g, replicas=n, lib_path=lib_path)
    with pytest.raises(ValueError, match="seeds"):
        Mgm2Engine(g, replicas=3, seeds=[1, 2], lib_path=lib_path)
    lib = load_library(lib_path)
    cg, cp = g.to_c(), Params().to_c()
    seeds = np.arange(4097, dtype=np.uint64)
    for n in (0, 4097, -3):
        h = C.c_void_p()
        rc = lib.mxs_mgm2_create_replicas(C.byref(cg), C.byref(cp), None, 0.5, 0, seeds.ctypes.data, n, 0, C.byref(h))
        assert rc == MXS_E_INVALID and not h.value, n
    h = C.c_void_p()
    assert lib.mxs_mgm2_create_replicas(C.byref(cg), C.byref(cp), None, 0.5, 0, None, 2, 0, C.byref(h)) == MXS_E_INVALID
    assert "seeds" in lib.mxs_last_error().decode()
    with Mgm2Engine(g, replicas=2, lib_path=lib_path) as e:
        for r in (-1, 2):
            with pytest.raises(MaxSumGpuError, match="replica"):
                e.state(r)


@pytest.mark.parametrize("path", mgm2_golden_files(), ids=lambda p: os.path.basename(p)[:-4])
def test_reference_fixtures(path, lib_path):
    g, pkw, kw, rounds, ref_idx, ref_cost = load_mgm2_golden(path)
    kw = dict(kw)
    seed = int(kw.pop("seed"))
    with Mgm2Engine(g, Params(**pkw), seeds=[seed + 1, seed], replicas=2, lib_path=lib_path, **kw) as eng:
        eng.run(rounds)
        check_golden(eng.state(1), ref_idx, ref_cost)


def test_fixture_set_is_complete():
    assert len(mgm2_golden_files()) == 14


def test_device_costs_and_the_best_replica(lib_path):
    """on the hard colouring (integer tables, no variable costs) with infinity = 1000 both numbers are exact; best() is
    the winner derived from the oracle's final states alone"""
    g = G.random_coloring(45, seed=31, variant="hard", unary_noise=0)
    seeds, kw = list(range(5, 13)), dict(favor="coordinated")
    finals = oracle_finals(g, Params(), kw, seeds, 12, 1000.0)
    assert [f[0] for f in finals] == [4, 5, 4, 4, 4, 5, 3, 5] and all(f[1] == 0 for f in finals)
    w = winner(finals, False)
    assert w == 6 and sum(f[:2] == finals[w][:2] for f in finals) == 1      # something to rank, a unique winner
    with Mgm2Engine(g, Params(), seeds=seeds, replicas=len(seeds), lib_path=lib_path, **kw) as eng:
        for n in (0, 12):
            eng.run(n)
            cost, viol = check_costs(eng, range(len(seeds)), infinity=1000.0)
            for r in range(len(seeds)):
                assert (cost[r], viol[r]) == eng.eval_cost(eng.assignment(r)[0], 1000.0)
        for r, (v, c, idx) in enumerate(finals):
            assert (viol[r], cost[r]) == (v, c)
        b = eng.best(1000.0)
        assert (b["replica"], b["violations"], b["cost"]) == (w, finals[w][0], finals[w][1])
        np.testing.assert_array_equal(b["idx"], finals[w][2])
    # max mode, float tables and variable costs: the cost to rounding, the ranking on the negated cost
    g = G.random_coloring(40, seed=33)
    with Mgm2Engine(g, Params(mode="max"), seed=3, replicas=6, lib_path=lib_path) as eng:
        eng.run(8)
        cost, viol = check_costs(eng, range(6))
        b = eng.best()
        assert b["replica"] == winner([(viol[r], cost[r]) for r in range(6)], True)
        assert len(set(cost)) > 1
