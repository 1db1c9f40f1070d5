"""GDBA replicas (GdbaEngine(replicas=R): R seeded runs in one engine, pydcop_amd/csrc/gdba.h) against
tests/gdba_oracle.py: replica r is bit for bit OracleGdba(seed=seeds[r]), modifier tables included; the device cost
against eval_cost; the best-state records against records derived from the oracle alone; the fixtures recorded from the
reference (tests/golden/gdba).  The test functions live here, below the helpers; tests/test_gdba_replicas_emu.py
(emulated build) and tests/test_gpu_gdba_replicas.py (the HIP library) import them and provide the `lib_path` fixture,
so the two runs cannot drift apart."""
import ctypes as C
import os

import numpy as np
import pytest

from dsa_replicas_common import better, check_costs, oracle_records, winner
from gdba_common import GENERAL, LIVE, check_golden, gdba_golden_files, load_gdba_golden
from gdba_oracle import OracleGdba
from mgm_common import shuffled_names
from pydcop_amd import generators as G
from pydcop_amd.engine import MaxSumGpuError, load_library
from pydcop_amd.gdba import GdbaEngine
from pydcop_amd.graph import Params

KEYS = ("idx", "has_cost", "cost", "improve", "new")
HARD = "hard150_T"
MXS_E_INVALID, MXS_E_STATE = -1, -5
STEPS = (0, 1, 1, 3, 7)                     # the states after 0, 1, 2, 5 and 12 rounds


def _named(pool, name):
    return dict(pool)[name]


def parity_cases():
    """(id, instance, Params kwargs, GDBA kwargs, R): the smallest shapes that cross each boundary"""
    return [
        # three variable blocks per replica, the last one partial; name-rank ties
        (HARD, lambda: shuffled_names(G.random_coloring(150, seed=63, variant="hard", unary_noise=0), 63), {},
         dict(modifier="A", violation="NZ", increase_mode="T"), 3),
        # one case per increase mode with stored tables, on instances with live slots
        ("E_matched_pairs_binary", _named(LIVE, "matched_pairs_binary"), {},
         dict(modifier="A", violation="NM", increase_mode="E"), 3),
        # (dyadic variable costs: slot_vc is per replica; a variable without neighbours)
        ("R_stars_paths_unaries", _named(LIVE, "stars_paths_unaries"), {},
         dict(modifier="A", violation="NM", increase_mode="R"), 3),
        # (arity 3, initial values: the same in every replica)
        ("C_triples_arity3_init", _named(LIVE, "triples_arity3_init"), {},
         dict(modifier="A", violation="NM", increase_mode="C"), 2),
        ("modifier_M", lambda: G.random_mixed(40, 70, seed=65, float_tables=False, unary_noise=0), {},
         dict(modifier="M", violation="NM", increase_mode="T"), 3),
        ("f32_max", _named(GENERAL, "repeated_pairs_unaries"), {"mode": "max", "dtype": "f32"},
         dict(modifier="A", violation="NZ", increase_mode="T"), 2),
        # float variable costs that are no dyadic fractions: the cumulative sums of every replica in index order
        ("variable_costs", lambda: G.random_mixed(40, 60, seed=7), {},
         dict(modifier="M", violation="NM", increase_mode="T"), 2),
        ("init_idx", _named(GENERAL, "hard_deg4_init"), {}, dict(modifier="A", violation="NZ", increase_mode="T"), 2),
        # variables without neighbours take their optimal_cost_value in every replica
        ("isolated_max", lambda: G.random_coloring(60, avg_degree=1, seed=36), {"mode": "max"},
         dict(modifier="A", violation="NZ", increase_mode="E"), 5),
    ]


def n_slots(graph):
    return len(graph.var_edges)


def same_state(eng, oras, what):
    for r, ora in oras.items():
        se, so = eng.state(r), ora.state()
        for k in KEYS:
            np.testing.assert_array_equal(se[k], so[k], err_msg=f"{k} of replica {r} {what}")
        for s in range(n_slots(ora.graph)):
            np.testing.assert_array_equal(eng.modifiers(s, replica=r), ora.modifiers(s),
                                          err_msg=f"modifiers of slot {s} of replica {r} {what}")


def compare_replicas(graph, params, kw, replicas, lib_path=None, seed=5, seeds=None, check=None, steps=STEPS):
    """every replica of `check` (default: all) against OracleGdba(seed=seeds[r]): idx, has_cost, cost, improve, new and
    every stored modifier table bit for bit after 0, 1, 2, 5 and 12 rounds, then after reset() and 5 rounds.  Returns
    the engine (after those 5 rounds), the oracles' start states, their states after the steps and their modifier
    tables after the steps."""
    eng = GdbaEngine(graph, params, seed=seed, seeds=seeds, replicas=replicas, lib_path=lib_path, **kw)
    assert eng.replicas == replicas and len(eng.seeds) == replicas
    if seeds is None:
        assert eng.seeds == [seed + r for r in range(replicas)]
    check = list(range(replicas)) if check is None else list(check)
    oras = {r: OracleGdba(graph, params, seed=eng.seeds[r], **kw) for r in check}
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
    mods = {r: [o.modifiers(s) for s in range(n_slots(graph))] for r, o in oras.items()}
    eng.reset()
    assert eng.cycle_count == 0
    for ora in oras.values():
        ora.reset()
    same_state(eng, oras, "after reset()")
    eng.run(5)
    for ora in oras.values():
        ora.run(5)
        assert eng.cycle_count == ora.cycle_count == 5
    same_state(eng, oras, "after reset() and 5 rounds")
    # replica 0 is what the single-state calls mean
    np.testing.assert_array_equal(eng.assignment()[0], eng.assignment(0)[0])
    assert eng.eval_cost() == eng.eval_cost(eng.assignment(0)[0])
    assert eng.pool_bytes == 2 * replicas * sum(len(m) for m in mods[check[0]])   # the whole pool, all replicas
    return eng, starts, finals, mods


class ReplicaView:
    """what check_golden reads of an engine, of one replica"""

    def __init__(self, eng, replica):
        self.eng, self.replica = eng, replica

    def state(self):
        return self.eng.state(self.replica)

    def modifiers(self, slot):
        return self.eng.modifiers(slot, replica=self.replica)


# ---- best state: the instance of the issue's measurement

BEST_SEEDS = list(range(5, 11))
BEST_ROUNDS = 30
BEST_KW = dict(modifier="M", violation="NM", increase_mode="T")


def best_instance():
    return G.random_mixed(40, 70, seed=65, float_tables=False, unary_noise=0)


def best_records(every, infinity=float("inf")):
    """(records, finals) of the six runs from the oracle alone (dsa_replicas_common.oracle_records: stepped one round
    at a time with the oracle's own eval_cost)"""
    return oracle_records(OracleGdba, best_instance(), Params(), BEST_KW, BEST_SEEDS, BEST_ROUNDS, every, infinity)


def assert_records_are_not_the_final_states(records, finals, every):
    """(the oracle side) what keeps the comparison from passing with the final state returned as the record"""
    differ = [r for r in range(len(records)) if (records[r][3] != finals[r][2]).any()]
    early = [r for r in range(len(records)) if records[r][2] < BEST_ROUNDS]
    assert len(differ) >= 4, f"every={every}: the record differs from the final state in {len(differ)} of 6 runs only"
    assert len(early) >= 4, f"every={every}: the record's round is below {BEST_ROUNDS} in {len(early)} of 6 runs only"
    assert not any(better(finals[r][:2], records[r][:2], False) for r in range(len(records)))


# ---- the tests; `lib_path`: the fixture of the importing file (the emulated build, or None = the HIP library)

@pytest.mark.parametrize("case", parity_cases(), ids=lambda c: c[0])
def test_every_replica_equals_the_oracle(case, lib_path):
    name, make, pkw, kw, replicas = case
    eng, starts, finals, mods = compare_replicas(make(), Params(**pkw), kw, replicas, lib_path=lib_path)
    eng.close()
    if name == HARD:
        # what keeps the comparison from passing with the replica fold left out, or with one pool for all replicas
        # (conditions on the oracle side): the runs start apart and end apart, a modifier table differs
        assert all((starts[r] != starts[0]).any() for r in starts if r)
        assert all((finals[r] != finals[0]).any() for r in finals if r)
        assert any((a != b).any() for a, b in zip(mods[0], mods[1]))


def test_many_small_replicas(lib_path):
    """more blocks than one replica needs, and the highest offsets: 64 replicas of 12 variables"""
    eng, *_ = compare_replicas(G.random_coloring(12, seed=31, variant="hard"), Params(),
                               dict(modifier="A", violation="NZ", increase_mode="T"), 64, lib_path=lib_path,
                               check=(0, 1, 31, 32, 63))
    eng.close()


def test_explicit_seeds(lib_path):
    seeds = [9, 9, 2 ** 64 - 1, 2 ** 63]
    g = G.random_coloring(45, seed=31, variant="hard")
    eng, *_ = compare_replicas(g, Params(), dict(modifier="M", violation="NZ", increase_mode="T"), 4, lib_path=lib_path,
                               seeds=seeds)
    assert eng.seeds == seeds
    s0, s1 = eng.state(0), eng.state(1)
    for k in KEYS:                                                 # the same seed: the same run, modifiers included
        np.testing.assert_array_equal(s0[k], s1[k])
    tables = [eng.modifiers(s, replica=0) for s in range(n_slots(g))]
    for s in range(n_slots(g)):
        np.testing.assert_array_equal(tables[s], eng.modifiers(s, replica=1))
    assert any((t != 1).any() for t in tables)                     # (and something was increased)
    eng.close()
    with GdbaEngine(G.random_coloring(10, seed=1), seed=2 ** 64 - 1, replicas=2, lib_path=lib_path) as e:
        assert e.seeds == [2 ** 64 - 1, 0]                         # the default seeds wrap modulo 2**64


def test_one_replica_equals_the_single_run_engine(lib_path):
    """seeds=[s] goes through mxs_gdba_create_replicas, seed=s through mxs_gdba_create: the same run, the oracle's"""
    g, s = shuffled_names(G.random_coloring(80, seed=63, variant="hard"), 63), 11
    kw = dict(modifier="A", violation="NZ", increase_mode="T")
    with GdbaEngine(g, Params(), seeds=[s], replicas=1, lib_path=lib_path, **kw) as rep, \
            GdbaEngine(g, Params(), seed=s, lib_path=lib_path, **kw) as one:
        n = C.c_int32(0)
        for e in (rep, one):
            e._call("replicas", C.byref(n))
            assert n.value == 1 and e.replicas == 1 and e.seeds == [s]
        ora = OracleGdba(g, Params(), seed=s, **kw)
        for n_rounds in (0, 1, 6):
            rep.run(n_rounds), one.run(n_rounds), ora.run(n_rounds)
            for k in KEYS:
                np.testing.assert_array_equal(rep.state()[k], one.state()[k])
                np.testing.assert_array_equal(rep.state()[k], ora.state()[k])
            for sl in range(n_slots(g)):
                np.testing.assert_array_equal(rep.modifiers(sl), one.modifiers(sl))
                np.testing.assert_array_equal(rep.modifiers(sl), ora.modifiers(sl))
        assert rep.pool_bytes == one.pool_bytes
        # one run's replica costs are its eval_cost; the replica engine's are the device's sum of the same items
        (c1, v1), (cr, vr) = one.replica_costs(1000.0), rep.replica_costs(1000.0)
        assert (c1[0], v1[0]) == one.eval_cost(infinity=1000.0) and vr[0] == v1[0] and v1[0] > 0
        assert abs(cr[0] - c1[0]) <= 1e-9 * max(1.0, abs(c1[0]))
        with pytest.raises(MaxSumGpuError, match="replica"):
            one.state(1)
        with pytest.raises(MaxSumGpuError, match="replica"):
            rep.state(1)


@pytest.mark.parametrize("path", gdba_golden_files(), ids=lambda p: os.path.basename(p)[:-4])
def test_reference_fixtures(path, lib_path):
    g, pkw, kw, rounds, ref = load_gdba_golden(path)
    kw = dict(kw)
    seed = int(kw.pop("seed"))
    with GdbaEngine(g, Params(**pkw), seeds=[seed + 1, seed], replicas=2, lib_path=lib_path, **kw) as eng:
        eng.run(rounds)
        check_golden(ReplicaView(eng, 1), ref)


def test_fixture_set_is_complete():
    assert len(gdba_golden_files()) == 50


@pytest.mark.parametrize("every", [1, 3])
def test_best_state_records_equal_the_oracle_derived_ones(every, lib_path):
    """M / NM / T on the integer mixed instance, seeds 5..10, 30 rounds: the tables are integers and there are no
    variable costs, so every cost is exact and the device ranking cannot differ from the host's.  Measured on the
    oracle: at every = 1 the record differs from the final state in 6 of 6 runs (e.g. seed 5: cost 179 at round 3,
    final cost 214), the winner is replica 4 with cost 173."""
    g, params, inf = best_instance(), Params(), float("inf")
    records, finals = best_records(every)
    assert_records_are_not_the_final_states(records, finals, every)
    w = winner(records, False)
    if every == 1:
        assert sum(rec[:2] == records[w][:2] for rec in records) == 1          # a unique winner
        assert (w, records[w][1]) == (4, 173.0) and (records[0][1], records[0][2], finals[0][1]) == (179.0, 3, 214.0)
    R = len(BEST_SEEDS)
    with GdbaEngine(g, params, seeds=BEST_SEEDS, replicas=R, lib_path=lib_path, **BEST_KW) as eng:
        eng.track_best(every, inf)
        eng.run(10), eng.run(BEST_ROUNDS - 10)          # (records live across calls of run)

        def same_records():
            for r, (viol, cost, rnd, idx) in enumerate(records):
                b = eng.best(r)
                assert (b["replica"], b["violations"], b["cost"], b["cycle"]) == (r, viol, cost, rnd), (r, b, records[r][:3])
                np.testing.assert_array_equal(b["idx"], idx, err_msg=f"snapshot of replica {r}")
            b = eng.best()
            assert (b["replica"], b["violations"], b["cost"], b["cycle"]) == (w,) + records[w][:3]
            np.testing.assert_array_equal(b["idx"], records[w][3])

        same_records()
        # the current states: replica_costs is eval_cost of every replica's assignment, and the oracle's final cost
        cost, viol = check_costs(eng, range(R), infinity=inf)
        for r in range(R):
            assert (cost[r], viol[r]) == eng.eval_cost(eng.assignment(r)[0], inf) == (finals[r][1], finals[r][0])
            np.testing.assert_array_equal(eng.assignment(r)[0], finals[r][2])
        # reset() clears the records: the same run gives the same records again, not better ones
        eng.reset()
        b0 = eng.best(0)
        assert b0["cycle"] == 0 and np.array_equal(b0["idx"], eng.assignment(0)[0])
        eng.run(BEST_ROUNDS)
        same_records()
        # track_best again clears them: the record is the state as it is now
        eng.track_best(every, inf)
        for r in range(R):
            b = eng.best(r)
            assert (b["violations"], b["cost"], b["cycle"]) == (finals[r][0], finals[r][1], BEST_ROUNDS)
            np.testing.assert_array_equal(b["idx"], finals[r][2])
        # tracking off: best() ranks the current states
        eng.track_best(0, inf)
        b = eng.best()
        assert b["replica"] == winner(finals, False) and b["cycle"] == BEST_ROUNDS
        assert (b["violations"], b["cost"]) == finals[b["replica"]][:2]
        np.testing.assert_array_equal(b["idx"], finals[b["replica"]][2])


SPAN_SEEDS = [5, 6, 7, 8]
SPAN_ROUNDS = 40
SPAN_BLOCK = 256                            # the copy kernel's block: index >= 256 is its second block


@pytest.mark.parametrize("every", [1, 4])
def test_gdba_best_state_snapshots_span_blocks(every, lib_path):
    """300 variables: two blocks of repcost::k_best_copy per replica, the smallest size with a second block.  M / NM /
    T on the hard colouring (integer tables, no variable costs: every cost is exact), seeds 5..8, 40 rounds, infinity
    1000.  Measured on the oracle: the records are of rounds 21 / 32 / 33 / 40 (every = 1) and 20 / 32 / 32 / 40
    (every = 4); those of seeds 5 and 6 differ from the run's final state at 7 and 3 indices >= 256."""
    g, params, inf = G.random_coloring(300, seed=32, variant="hard", unary_noise=0), Params(), 1000.0
    records, finals = oracle_records(OracleGdba, g, params, BEST_KW, SPAN_SEEDS, SPAN_ROUNDS, every, inf)
    # the oracle side: a snapshot that missed its second block (the final state left there) would be seen
    beyond = [int((rec[3][SPAN_BLOCK:] != fin[2][SPAN_BLOCK:]).sum()) for rec, fin in zip(records, finals)]
    assert sum(n > 0 for n in beyond) >= 2, f"every={every}: records differ from the final states past index 256 in {beyond}"
    assert [rec[2] for rec in records] == {1: [21, 32, 33, 40], 4: [20, 32, 32, 40]}[every]
    w = winner(records, False)
    with GdbaEngine(g, params, seeds=SPAN_SEEDS, replicas=len(SPAN_SEEDS), lib_path=lib_path, **BEST_KW) as eng:
        eng.track_best(every, inf)
        for _ in range(2):
            eng.run(SPAN_ROUNDS)
            for r, (viol, cost, rnd, idx) in enumerate(records):
                b = eng.best(r)
                assert (b["replica"], b["violations"], b["cost"], b["cycle"]) == (r, viol, cost, rnd), (r, b, records[r][:3])
                np.testing.assert_array_equal(b["idx"], idx, err_msg=f"snapshot of replica {r}")
            b = eng.best()
            assert (b["replica"], b["violations"], b["cost"], b["cycle"]) == (w,) + records[w][:3]
            np.testing.assert_array_equal(b["idx"], records[w][3])
            eng.reset()                     # the records start again: the same run gives the same records


def test_device_costs_in_max_mode_with_float_tables(lib_path):
    """float tables and variable costs: the cost to rounding (check_costs), the ranking on the negated cost"""
    g = G.random_coloring(40, seed=33)
    kw = dict(modifier="A", violation="NZ", increase_mode="T")
    with GdbaEngine(g, Params(mode="max"), seed=3, replicas=6, lib_path=lib_path, **kw) as eng:
        eng.track_best(2)
        eng.run(8)
        cost, viol = check_costs(eng, range(6))
        assert len(set(cost)) > 1
        recs = [eng.best(r) for r in range(6)]
        for r, b in enumerate(recs):                    # a record is never worse than the current state
            assert b["cycle"] % 2 == 0 and not better((viol[r], cost[r]), (b["violations"], b["cost"]), True)
            c, v = eng.eval_cost(b["idx"])
            assert v == b["violations"] and abs(c - b["cost"]) <= 1e-9 * max(1.0, abs(c))
        assert eng.best()["replica"] == winner([(b["violations"], b["cost"]) for b in recs], True)
        eng.track_best(0)
        assert eng.best()["replica"] == winner([(viol[r], cost[r]) for r in range(6)], True)


def test_refusals(lib_path):
    g = G.random_coloring(12, seed=1)
    for n in (0, 4097):
        with pytest.raises(MaxSumGpuError, match=f"error {MXS_E_INVALID}: .*replicas"):
            GdbaEngine(g, replicas=n, lib_path=lib_path)
    with pytest.raises(ValueError, match="seeds"):
        GdbaEngine(g, replicas=3, seeds=[1, 2], lib_path=lib_path)
    lib = load_library(lib_path)
    cg, cp = g.to_c(), Params().to_c()
    seeds = np.arange(4097, dtype=np.uint64)
    for n in (0, 4097, -3):
        h = C.c_void_p()
        rc = lib.mxs_gdba_create_replicas(C.byref(cg), C.byref(cp), None, None, 0, 0, 0, seeds.ctypes.data, n, 0, 0,
                                          C.byref(h))
        assert rc == MXS_E_INVALID and not h.value, n
    h = C.c_void_p()
    assert lib.mxs_gdba_create_replicas(C.byref(cg), C.byref(cp), None, None, 0, 0, 0, None, 2, 0, 0,
                                        C.byref(h)) == MXS_E_INVALID and not h.value
    assert "seeds" in lib.mxs_last_error().decode()
    # a pool budget that admits one replica and not three
    sparse = G.random_coloring(20, avg_degree=1, seed=1)
    with GdbaEngine(sparse, Params(), increase_mode="C", lib_path=lib_path) as e:
        need = e.pool_bytes
    assert need > 0
    with GdbaEngine(sparse, Params(), increase_mode="C", seeds=[4], pool_budget=need, lib_path=lib_path) as e:
        assert e.pool_bytes == need
    with pytest.raises(MaxSumGpuError, match=f"error {MXS_E_INVALID}: .*3 replicas take {3 * need} bytes.*budget of {3 * need - 1}"):
        GdbaEngine(sparse, Params(), increase_mode="C", replicas=3, pool_budget=3 * need - 1, lib_path=lib_path)
    with GdbaEngine(sparse, Params(), increase_mode="C", replicas=3, pool_budget=3 * need, lib_path=lib_path) as e:
        assert e.pool_bytes == 3 * need
    with GdbaEngine(g, replicas=2, lib_path=lib_path) as e:
        with pytest.raises(MaxSumGpuError, match=f"error {MXS_E_STATE}: .*track_best"):
            e.best()
        with pytest.raises(MaxSumGpuError, match=f"error {MXS_E_INVALID}: .*every"):
            e.track_best(-1)
        e.track_best(1)
        for r in (-1, 2):
            with pytest.raises(MaxSumGpuError, match="replica"):
                e.state(r)
            with pytest.raises(MaxSumGpuError, match="replica"):
                e.modifiers(0, replica=r)
        for r in (-2, 2):
            with pytest.raises(MaxSumGpuError, match="replica"):
                e.best(r)
    # the single-run engine keeps no records
    with GdbaEngine(g, lib_path=lib_path) as e:
        with pytest.raises(MaxSumGpuError, match=f"error {MXS_E_STATE}"):
            e.best()
        with pytest.raises(MaxSumGpuError, match=f"error {MXS_E_STATE}"):
            e.track_best(1)
