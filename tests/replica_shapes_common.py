"""The replica engines (DsaEngine, MgmEngine(draws="keyed"), Mgm2Engine, GdbaEngine with replicas=R) at the shapes where a
launch spans several blocks per replica: two and three blocks of k_cost_partial (1024 items each), a second and a third block
of k_cost_final (64 replicas each), init and snapshot kernels over more than 256 variables, the packed and the
thread-per-variable kernels of one cycle with different numbers of blocks per replica, the top of the replica range.
Replica r is bit for bit its single-seed oracle (GDBA: its stored modifier tables too, so that the pool
[replicas][n_pool] is read at several blocks per replica as well); every replica's device cost is checked against the
plain Python sum of tests/replica_cost_reference.py; ranking ties break on the lowest index; GDBA's best-state records
of replicas past the first block of k_cost_final.  The test functions live here, below the
helpers; tests/test_replica_shapes_emu.py (emulated build: blocks one after another) and
tests/test_gpu_replica_shapes.py (the HIP library: a real grid) import them and provide the `lib_path` fixture."""
import numpy as np
import pytest

import dsa_replicas_common as dsar
import gdba_replicas_common as gdbar
import mgm2_replicas_common as mgm2r
import mgm_replicas_common as mgmr
from gdba_oracle import OracleGdba
from mgm2_oracle import OracleMgm2
from mgm_keyed_oracle import OracleMgmKeyed
from pydcop_amd import generators as G
from pydcop_amd.dsa import DsaEngine
from pydcop_amd.gdba import GdbaEngine
from pydcop_amd.graph import Params
from pydcop_amd.mgm import MgmEngine
from pydcop_amd.mgm2 import Mgm2Engine
from replica_cost_reference import (CHUNK, INF, acceptable_winners, assert_chunks_carry_weight,
                                    assert_chunks_hold_violations, check_replica_costs, cost_bound, is_exact,
                                    reference_cost)

GENERIC = "MAXSUM_LOCAL_SEARCH_GENERIC"
STEPS = (0, 1, 3)            # compared after rounds 0, 1 and 4, then after reset() and RESET_ROUNDS
RESET_ROUNDS = 2


# ---- the engines under one face: engine, single-seed oracle, the fields compared bit for bit; "tracked": best() is
# the tracker's (track_best(0, infinity) first), else the ranking of the current states (best(infinity)); "tables":
# the stored modifier tables of every slot are compared too; "tie_kw": the engine's keywords in the tie test

def dsa_oracle(g, p, kw, seed):
    from oracle.dsa_oracle import OracleDsa
    return OracleDsa(g, p, seed=seed, **kw)


def dsa_fields(x):
    idx, cost = x.assignment() if not isinstance(x, tuple) else x
    return {"idx": idx, "cost": cost}


ENGINES = {
    "dsa": dict(engine=lambda g, p, kw, **rep: DsaEngine(g, p, **kw, **rep), oracle=dsa_oracle,
                fields=lambda eng, r: dsa_fields(eng.assignment(r)), ora_fields=dsa_fields, kw="dsa", tracked=True),
    "mgm": dict(engine=lambda g, p, kw, **rep: MgmEngine(g, p, draws="keyed", **rep),
                oracle=lambda g, p, kw, seed: OracleMgmKeyed(g, p, draws="keyed", seed=seed),
                fields=lambda eng, r: {k: eng.state(r)[k] for k in mgmr.KEYS},
                ora_fields=lambda o: {k: o.state()[k] for k in mgmr.KEYS}, kw=None),
    "mgm2": dict(engine=lambda g, p, kw, **rep: Mgm2Engine(g, p, **kw, **rep),
                 oracle=lambda g, p, kw, seed: OracleMgm2(g, p, seed=seed, **kw),
                 fields=lambda eng, r: {k: eng.state(r)[k] for k in mgm2r.KEYS},
                 ora_fields=lambda o: {k: o.state()[k] for k in mgm2r.KEYS}, kw="mgm2"),
    "gdba": dict(engine=lambda g, p, kw, **rep: GdbaEngine(g, p, **kw, **rep),
                 oracle=lambda g, p, kw, seed: OracleGdba(g, p, seed=seed, **kw),
                 fields=lambda eng, r: {k: eng.state(r)[k] for k in gdbar.KEYS},
                 ora_fields=lambda o: {k: o.state()[k] for k in gdbar.KEYS}, kw="gdba", tracked=True, tables=True,
                 tie_kw=dict(modifier="A", violation="NZ", increase_mode="T")),
}
# GDBA once more with the second keyword set of a case (stored tables: pool [replicas][n_pool])
ENGINES["gdba_stored"] = dict(ENGINES["gdba"], kw="gdba_stored")


def same_fields(E, eng, oras, what):
    for r, ora in oras.items():
        got, want = E["fields"](eng, r), E["ora_fields"](ora)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k} of replica {r} {what}")
        if E.get("tables"):
            for s in range(gdbar.n_slots(ora.graph)):
                np.testing.assert_array_equal(eng.modifiers(s, replica=r), ora.modifiers(s),
                                              err_msg=f"modifiers of slot {s} of replica {r} {what}")


def eval_costs_instance():
    """variable costs for the evaluation that differ from the ones the algorithm reads, by far more than any bound"""
    g = G.random_coloring(300, seed=33)
    g.eval_var_cost = 1.0 + g.var_cost[::-1].copy()
    return g


def two_cost_blocks():
    return G.random_coloring(450, seed=31)


def small_hard():
    return G.random_coloring(12, seed=31, variant="hard")


# id -> (instance, Params kwargs, {"dsa": DSA kwargs, "mgm2": MGM-2 kwargs, "gdba", "gdba_stored": GDBA kwargs}, infinity,
# R, compared replicas or None = all, kind, environment, engines); kind: "float" real-valued tables, "hard" 0 / 1000
# tables, "costs" integer tables and real-valued variable costs.
# GDBA: increase mode T wherever the instance has real-valued variable costs (the reference sums them in set order in the
# other modes: gdba_oracle.py, Determinism); on the instance without any a second run with stored tables.  GDBA has no
# $MAXSUM_LOCAL_SEARCH_GENERIC path (gdba.h reads no environment): the two forced cases stay DSA's and MGM's.
ALL = ("dsa", "mgm", "mgm2", "gdba")
GDBA_T = dict(modifier="A", violation="NZ", increase_mode="T")
GDBA_KW = {"gdba": GDBA_T}
CASES = {
    # 1350 items: the second cost block holds 326; 2 init blocks, 8 blocks of the thread-per-variable kernels
    "two_cost_blocks": (two_cost_blocks, {}, GDBA_KW, INF, 3, None, "costs", {}, ALL),
    # 2100 items: 3 partials, the third of variables alone; violations exact, the cost exactly 0
    # (GDBA with stored tables: 2800 slots of 9 entries, 25200 pool entries per replica)
    "three_cost_blocks_hard": (lambda: G.random_coloring(700, seed=32, variant="hard", unary_noise=0), {},
                               {"gdba": dict(modifier="M", violation="NM", increase_mode="T"),
                                "gdba_stored": dict(modifier="M", violation="NZ", increase_mode="E")}, 1000.0, 2,
                               None, "hard", {}, ALL + ("gdba_stored",)),
    # 1100 items, tables that are not f32-exact; packed and rest kernels, each with its own blocks per replica
    "mixed_f32_max": (lambda: G.random_mixed(300, 800, seed=34, dom_choices=(2, 3, 4)), {"mode": "max", "dtype": "f32"},
                      {"dsa": dict(p_mode="arity"), "gdba": dict(modifier="M", violation="NM", increase_mode="T")}, INF, 3, None,
                      "float", {}, ALL),
    "eval_var_cost": (eval_costs_instance, {"mode": "max"}, GDBA_KW, INF, 2, None, "costs", {}, ALL),
    # a second and a third block of k_cost_final
    "many_replicas": (small_hard, {}, GDBA_KW, 1000.0, 130, (0, 63, 64, 65, 129), "hard", {}, ALL),
    # the top of the replica range
    "replica_limit": (small_hard, {}, GDBA_KW, 1000.0, 4096, (0, 64, 4095), "hard", {}, ALL),
    # the slot and the CSR-walk kernels at several blocks per replica
    "forced_generic_1": (two_cost_blocks, {}, {}, INF, 2, None, "costs", {GENERIC: "1"}, ("dsa", "mgm")),
    "forced_generic_2": (two_cost_blocks, {}, {}, INF, 2, None, "costs", {GENERIC: "2"}, ("dsa", "mgm")),
}


LIMIT = "replica_limit"      # on the GPU alone: the emulated build takes 8 s (MGM-2) to 80 s (MGM) for its 4096 x 5 blocks a round


def shape_params():
    return [pytest.param(name, e, id=f"{name}-{e}") for name, c in CASES.items() for e in c[8] if name != LIMIT]


def check_all_costs(eng, graph, params, infinity, kind, compared):
    """every replica's device cost against the reference; on the compared replicas what keeps that from being vacuous
    (the reference side alone)"""
    refs = check_replica_costs(eng, range(eng.replicas), infinity)
    for r in compared:
        idx = eng.assignment(r)[0]
        if kind == "hard":
            assert_chunks_hold_violations(graph, params, idx, infinity)
            if not graph.var_cost.any():
                assert refs[r][0] == 0.0
        else:
            assert_chunks_carry_weight(graph, params, idx, infinity, runs=kind == "float")
    return refs


def compare_shape(name, engine, lib_path):
    make, pkw, kws, infinity, replicas, check, kind, env, _ = CASES[name]
    E = ENGINES[engine]
    graph, params, kw = make(), Params(**pkw), kws.get(E["kw"], {})
    eng = E["engine"](graph, params, kw, seed=5, replicas=replicas, lib_path=lib_path)
    assert eng.replicas == replicas
    check = list(range(replicas)) if check is None else list(check)
    oras = {r: E["oracle"](graph, params, kw, eng.seeds[r]) for r in check}
    done = 0
    for n in STEPS:
        eng.run(n)
        done += n
        for ora in oras.values():
            ora.run(n)
            assert eng.cycle_count == ora.cycle_count == done
        same_fields(E, eng, oras, f"after {done} rounds")
        refs = check_all_costs(eng, graph, params, infinity, kind, check)
    if name == LIMIT:
        if E.get("tracked"):
            eng.track_best(0, infinity)
        b = eng.best() if E.get("tracked") else eng.best(infinity)
        w, ok = acceptable_winners([refs[r] for r in range(replicas)], params.mode == "max", is_exact(graph, params))
        assert b["replica"] in ok, (b["replica"], w, ok)
        np.testing.assert_array_equal(b["idx"], refs[b["replica"]][4])
    if name == "eval_var_cost":      # the reference side: reading var_cost instead would be seen
        idx, plain = eng.assignment(0)[0], make()
        plain.eval_var_cost = None
        ref, other = refs[0], reference_cost(plain, params, idx, infinity)
        assert abs(ref[0] - other[0]) > 1000.0 * cost_bound(ref[3], max(ref[2], other[2]))
    if name == "mixed_f32_max":      # the reference side: the f64 tables' cost would be seen
        ref, other = refs[0], reference_cost(graph, Params(mode="max"), eng.assignment(0)[0], infinity)
        assert abs(ref[0] - other[0]) > 1000.0 * cost_bound(ref[3], max(ref[2], other[2]))
    eng.reset()
    eng.run(RESET_ROUNDS)
    for ora in oras.values():
        ora.reset(), ora.run(RESET_ROUNDS)
    same_fields(E, eng, oras, f"after reset() and {RESET_ROUNDS} rounds")
    check_all_costs(eng, graph, params, infinity, kind, check)
    eng.close()
    for ora in oras.values():
        ora.close()


# ---- the best state across blocks (DSA): 300 variables, two blocks of repcost::k_best_copy

def best_cases():
    soft = lambda: G.random_coloring(300, seed=31, unary_noise=0)                      # noqa: E731
    hard = lambda: G.random_coloring(300, seed=32, variant="hard", unary_noise=0)      # noqa: E731
    return [("soft300_A_every1", soft, {}, dict(variant="A", probability=1.0), INF, 1),
            ("hard300_C_every4", hard, {}, dict(variant="C", probability=0.9), 1000.0, 4)]


# ---- ties of the ranking

TIE_SEEDS = (5, 11, 6)
TIE_ROUNDS = 12


def tie_instance():
    return G.random_coloring(45, seed=31, variant="hard", unary_noise=0)


def tie_seeds(finals_of_seed, is_max):
    """From the oracle's final (violations, cost) of the three distinct seeds: the best seed at the indices 1 and 3, the
    others around it -- [worse, best, other, best, other].  The winner is index 1 unless the ranking prefers a later
    equal; index 0 must be strictly worse, or the lowest index would win whatever the rule."""
    order = sorted(TIE_SEEDS, key=lambda s: (finals_of_seed[s][0], -finals_of_seed[s][1] if is_max else finals_of_seed[s][1]))
    best, other, worst = order
    assert dsar.better(finals_of_seed[best], finals_of_seed[worst], is_max), "the three seeds end equally good"
    return [worst, best, other, best, other]


def compare_ties(engine, mode, lib_path):
    E, infinity = ENGINES[engine], 1000.0
    graph, params, kw = tie_instance(), Params(mode=mode), E.get("tie_kw", {})
    is_max = mode == "max"
    by_seed = {}
    for s in TIE_SEEDS:
        o = E["oracle"](graph, params, kw, s)
        o.run(TIE_ROUNDS)
        idx = E["ora_fields"](o)["idx"]
        c, v, _, _ = reference_cost(graph, params, idx, infinity)
        by_seed[s] = (v, c, np.array(idx))
        o.close()
    seeds = tie_seeds(by_seed, is_max)
    finals = [by_seed[s] for s in seeds]
    w = dsar.winner(finals, is_max)
    assert w == 1 and finals[1][:2] == finals[3][:2] and dsar.better(finals[1], finals[0], is_max)
    if engine == "gdba":             # (measured on the oracle, A / NZ / T)
        assert [f[0] for f in finals] == {"min": [7, 4, 6, 4, 6], "max": [38, 27, 32, 27, 32]}[mode]
    with E["engine"](graph, params, kw, seeds=seeds, replicas=len(seeds), lib_path=lib_path) as eng:
        eng.run(TIE_ROUNDS)
        cost, viol = eng.replica_costs(infinity)
        assert [(int(v), float(c)) for v, c in zip(viol, cost)] == [f[:2] for f in finals]
        if E.get("tracked"):
            eng.track_best(0, infinity)
            b = eng.best()
        else:
            b = eng.best(infinity)
        assert b["replica"] == 1, b
        assert (b["violations"], b["cost"]) == finals[1][:2]
        np.testing.assert_array_equal(b["idx"], finals[1][2])


# ---- the tests; `lib_path`: the fixture of the importing file (the emulated build, or None = the HIP library)

@pytest.mark.parametrize("name,engine", shape_params())
def test_replicas_equal_their_oracles_at_several_blocks(name, engine, oracle_built, monkeypatch, lib_path):
    for k, v in CASES[name][7].items():
        monkeypatch.setenv(k, v)
    compare_shape(name, engine, lib_path)


@pytest.mark.parametrize("engine", ALL)
def test_the_top_of_the_replica_range(engine, oracle_built, lib_path):
    """4096 replicas: three of them against their oracles, every cost against the reference, best() against the winner
    derived from the reference costs (tests/test_gpu_replica_shapes.py alone imports this one)"""
    compare_shape(LIMIT, engine, lib_path)


@pytest.mark.parametrize("case", best_cases(), ids=lambda c: c[0])
def test_best_state_snapshots_span_blocks(case, oracle_built, lib_path):
    from oracle.dsa_oracle import OracleDsa
    assert case[1]().n_vars > 256
    dsar.compare_best(OracleDsa, case, lib_path=lib_path)


@pytest.mark.parametrize("forced", [None, "1", "2"], ids=lambda f: f"generic{f or 0}")
def test_tracked_run_with_three_different_blocks_per_replica(forced, oracle_built, monkeypatch, lib_path):
    """450 variables, records after every cycle: the cost launch (2 blocks per replica) writes its number into the
    engine's kernel argument between the packed launch and the thread-per-variable launch (8 blocks per replica;
    forced: the CSR-walk and the slot kernels for every variable) of consecutive cycles.  A number left behind shows
    as a replica that leaves its oracle."""
    from oracle.dsa_oracle import OracleDsa
    if forced:
        monkeypatch.setenv(GENERIC, forced)
    graph, params, kw, replicas = two_cost_blocks(), Params(), dict(variant="B"), 3
    assert -(-(graph.n_factors + graph.n_vars) // CHUNK) == 2 and -(-graph.n_vars // 64) == 8
    E = ENGINES["dsa"]
    with DsaEngine(graph, params, seed=5, replicas=replicas, lib_path=lib_path, **kw) as eng:
        oras = {r: OracleDsa(graph, params, seed=5 + r, **kw) for r in range(replicas)}
        records = {r: None for r in oras}
        eng.track_best(1, INF)
        for cycle in range(7):
            if cycle:
                eng.run(1)
            for r, ora in oras.items():
                if cycle:
                    ora.run(1)
                idx = ora.assignment()[0].copy()
                c, v, _, _ = reference_cost(graph, params, idx)
                if records[r] is None or dsar.better((v, c), records[r][:2], False):
                    records[r] = (v, c, cycle, idx)
            same_fields(E, eng, oras, f"after {cycle} tracked cycles")
            refs = check_replica_costs(eng, range(replicas))       # (another cost launch before the next cycle)
            for r, (v, c, at, idx) in records.items():
                b = eng.best(r)
                assert (b["violations"], b["cycle"]) == (v, at), (r, b, records[r][:3])
                assert abs(b["cost"] - c) <= cost_bound(refs[r][3], refs[r][2])
                np.testing.assert_array_equal(b["idx"], idx, err_msg=f"snapshot of replica {r} after {cycle} cycles")
        assert any(rec[2] > 0 for rec in records.values())         # a record was replaced across the blocks
        for ora in oras.values():
            ora.close()


RECORD_ROUNDS = 12


def reference_records(graph, params, kw, seeds, rounds, infinity):
    """Per seed, from the oracle's states and reference_cost alone: the record (violations, cost, round, idx, sum of the
    items' magnitudes) of a run stepped one round at a time, replaced on strict improvement only; the final
    (violations, cost, idx); and whether every decision was clear -- two states of as many violations and different costs lie further apart than their two
    bounds, so that a sum in another order decides the same way."""
    is_max, exact = params.mode == "max", is_exact(graph, params)
    records, finals, clear = [], [], True
    for s in seeds:
        ora, rec = OracleGdba(graph, params, seed=s, **kw), None
        for c in range(rounds + 1):
            if c:
                ora.run(1)
            idx = ora.state()["idx"].copy()
            cost, viol, sum_abs, items = reference_cost(graph, params, idx, infinity)
            if rec is not None and not exact and viol == rec[0] and cost != rec[1]:
                clear = clear and abs(cost - rec[1]) > 2.0 * cost_bound(items, max(sum_abs, rec[4]))
            if rec is None or dsar.better((viol, cost), rec[:2], is_max):
                rec = (viol, cost, c, idx, sum_abs)
        records.append(rec)
        finals.append((viol, cost, idx))
        ora.close()
    return records, finals, clear


def test_gdba_best_state_records_beyond_the_first_block_of_the_final_reduction(lib_path):
    """130 replicas of small_hard() under track_best(1), 12 rounds: the `improved` flag and the record of a replica
    index of 64 or more (the second and third block of k_cost_final).  The records of replicas 0, 63, 64, 65 and 129,
    and best() against the winner over the records of all 130, derived from the oracle's states and reference_cost.
    Violations, round and snapshot are compared exactly; the cost to cost_bound (small_hard() has real-valued variable
    costs, which the device adds in its own order; exactly where is_exact).  M / NM / T, seeds 5..134; measured on
    the oracle: the records of replicas 63, 65 and 129 are of rounds 6, 9 and 2 and differ from the final states, 93 of
    the 130 records do."""
    graph, params, kw, inf, R = small_hard(), Params(), gdbar.BEST_KW, 1000.0, 130
    seeds, compared = [5 + r for r in range(R)], (0, 63, 64, 65, 129)
    records, finals, clear = reference_records(graph, params, kw, seeds, RECORD_ROUNDS, inf)
    assert clear, "a record's replacement hangs on a difference within the bound"
    # the oracle side: the final state returned as the record would be seen
    early = [r for r in compared if records[r][2] < RECORD_ROUNDS and (records[r][3] != finals[r][2]).any()]
    assert len(early) >= 2 and any(r >= 64 for r in early), early
    n, exact = graph.n_factors + graph.n_vars, is_exact(graph, params)
    bound = [0.0 if exact else cost_bound(n, rec[4]) for rec in records]
    w = dsar.winner(records, False)
    rivals = [r for r in range(R) if r != w and records[r][0] == records[w][0]
              and abs(records[r][1] - records[w][1]) <= 2.0 * (bound[r] + bound[w]) and (records[r][3] != records[w][3]).any()]
    assert not rivals, f"the winner {w} is not clear of {rivals}"
    with GdbaEngine(graph, params, seeds=seeds, replicas=R, lib_path=lib_path, **kw) as eng:
        eng.track_best(1, inf)
        eng.run(RECORD_ROUNDS)
        for asked, r in [(r, r) for r in compared] + [(-1, w)]:        # (-1: the best replica's record)
            viol, cost, rnd, idx, _ = records[r]
            b = eng.best(asked)
            assert (b["replica"], b["violations"], b["cycle"]) == (r, viol, rnd), (asked, b, viol, cost, rnd)
            assert abs(b["cost"] - cost) <= bound[r], (asked, b["cost"], cost, bound[r])
            np.testing.assert_array_equal(b["idx"], idx, err_msg=f"snapshot of replica {r}")


@pytest.mark.parametrize("mode", ["min", "max"])
@pytest.mark.parametrize("engine", ["dsa", "mgm", "mgm2", "gdba"])
def test_ranking_ties_break_on_the_lowest_index(engine, mode, oracle_built, lib_path):
    compare_ties(engine, mode, lib_path)
