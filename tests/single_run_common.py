"""The single-run engines of MGM-2 and GDBA (Mgm2Engine / GdbaEngine without `replicas` or `seeds`: mxs_mgm2_create,
mxs_gdba_create) through the paths they share with the replica engines: reset() is the device init kernel over one
replica, the static data is rephost::Host's, the rounds go through the plain entry points on the Dev part of the
replica argument (pydcop_amd/csrc/mgm2.h, gdba.h).  The test functions live here, below the helpers;
tests/test_single_run_emu.py (emulated build) and tests/test_gpu_single_run.py (the HIP library) import them and
provide the `lib_path` fixture, so the two runs cannot drift apart.  The comparison with the reference's semantics is
that of tests/gdba_common.py, tests/mgm2_common.py and tests/fuzz_common.py; here an engine is compared with itself
(fresh, after reset) and with the replica engine of the same seed."""
import numpy as np
import pytest

from mgm_common import unsorted_domains_with_ties, with_init
from pydcop_amd import generators as G
from pydcop_amd.engine import MaxSumGpuError
from pydcop_amd.gdba import GdbaEngine
from pydcop_amd.graph import FlatGraph, Params
from pydcop_amd.mgm2 import Mgm2Engine
from replica_cost_reference import check_replica_costs, cost_bound, reference_cost

INFINITY = 1000.0                       # the hard colourings' forbidden entries
MXS_E_INVALID, MXS_E_STATE = -1, -5
SEEDS = (3, 2 ** 64 - 2)


def no_variables():
    z32, z64 = np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64)
    return FlatGraph(dom_size=z32, var_cost=np.zeros(0), factor_rowptr=np.zeros(1, dtype=np.int32), edge_var=z32,
                     table_off=z64, tables=np.zeros(0), var_rowptr=np.zeros(1, dtype=np.int32), var_edges=z32)


def instances():
    """(id, instance, MGM-2 kwargs, GDBA kwargs).  12, 300 and 700 variables: one partial block of the init kernel
    (256 threads) and of the round kernels (64), then 2 and 5, then 3 and 11 -- the last ones partial; the start
    states the init kernel has to draw: initial values on some variables only, variables without neighbours whose
    cost ties break on the VALUE of an unsorted domain (GDBA: value_rank through start_values) or, for MGM-2, that
    draw among their best own values, variable costs that are no dyadic fractions, no variable at all."""
    return [
        ("vars_12", lambda: G.random_coloring(12, seed=31, variant="hard"), dict(favor="unilateral"),
         dict(modifier="A", violation="NZ", increase_mode="T")),
        ("vars_300", lambda: G.random_coloring(300, seed=63, variant="hard", unary_noise=0), dict(favor="coordinated"),
         dict(modifier="A", violation="NM", increase_mode="E")),
        ("vars_700", lambda: G.random_coloring(700, seed=64), dict(favor="no", threshold=0.7),
         dict(modifier="M", violation="NM", increase_mode="R")),
        ("init_on_some", lambda: with_init(G.random_coloring(90, seed=23, variant="hard"), 23), dict(favor="coordinated"),
         dict(modifier="A", violation="NZ", increase_mode="C")),
        ("isolated_unsorted_domains", lambda: unsorted_domains_with_ties(G.random_coloring(90, avg_degree=1, seed=32), 32),
         dict(favor="unilateral"), dict(modifier="A", violation="NZ", increase_mode="E")),
        ("isolated_unsorted_domains_max",
         lambda: unsorted_domains_with_ties(G.random_coloring(90, avg_degree=1, seed=33), 33), dict(favor="no"),
         dict(modifier="M", violation="MX", increase_mode="T")),
        ("variable_costs", lambda: G.random_mixed(40, 60, seed=7), dict(favor="coordinated"),
         dict(modifier="M", violation="NM", increase_mode="T")),
        ("no_variables", no_variables, dict(), dict()),
    ]


CASES = [pytest.param(algo, inst, dtype, id=f"{algo}-{inst[0]}-{dtype}")
         for algo in ("mgm2", "gdba") for inst in instances() for dtype in ("f64", "f32")]


def make(algo, inst, dtype, lib_path, **how):
    """-> (graph, params, a function that builds an engine on them)"""
    name, graph_of, mgm2_kw, gdba_kw = inst
    graph = graph_of()
    params = Params(dtype=dtype, mode="max" if name.endswith("_max") else "min")
    cls, kw = (Mgm2Engine, mgm2_kw) if algo == "mgm2" else (GdbaEngine, gdba_kw)
    return graph, params, lambda **more: cls(graph, params, lib_path=lib_path, **kw, **how, **more)


def snapshot(eng):
    """everything an engine shows of its dynamic state, as bytes: state() and, for GDBA, every stored modifier table"""
    out = {k: a.tobytes() for k, a in eng.state().items()}
    if isinstance(eng, GdbaEngine):
        for s in range(len(eng.graph.var_edges)):
            out[f"modifiers[{s}]"] = eng.modifiers(s).tobytes()
    return out


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], f"{k} differs {what}"


# ---- the tests; `lib_path`: the fixture of the importing file (the emulated build, or None = the HIP library)

@pytest.mark.parametrize("algo, inst, dtype", CASES)
def test_reset_gives_the_fresh_state_and_the_same_run(algo, inst, dtype, lib_path):
    graph, params, build = make(algo, inst, dtype, lib_path, seed=SEEDS[0])
    with build() as eng, build() as other:
        fresh = snapshot(eng)
        assert_same(snapshot(other), fresh, "between two fresh engines")
        if algo == "gdba" and graph.n_vars:             # the base of every stored modifier, nothing increased
            base = 1 if eng.modifier == "M" else 0
            assert all((eng.modifiers(s) == base).all() for s in range(len(graph.var_edges)))
        eng.run(5)
        first = snapshot(eng)
        assert eng.cycle_count == 5
        if graph.n_vars:                                # (the rounds did something: what reset() has to undo)
            assert first["has_cost"] != fresh["has_cost"] or first["idx"] != fresh["idx"]
        eng.reset()
        assert eng.cycle_count == 0
        assert_same(snapshot(eng), fresh, "after run(5) and reset()")
        eng.run(5)
        assert_same(snapshot(eng), first, "between run(5) and reset(), run(5)")


def test_the_start_states_have_the_shapes_the_cases_claim():
    """(the instances' side) what keeps the cases from passing on instances without the shape they are named for"""
    by_name = {i[0]: i[1]() for i in instances()}
    g = by_name["init_on_some"]
    assert (g.init_idx >= 0).any() and (g.init_idx < 0).any()
    for name in ("isolated_unsorted_domains", "isolated_unsorted_domains_max"):
        g = by_name[name]
        alone = np.setdiff1d(np.arange(g.n_vars), g.edge_var)
        off = g.cost_off
        ties = [v for v in alone if len(set(g.var_cost[off[v]:off[v + 1]])) < g.dom_size[v]]
        assert len(ties) >= 3 and g.value_rank() is not None
    g = by_name["variable_costs"]
    assert g.var_cost.any() and (g.var_cost * 2 ** 20 != np.floor(g.var_cost * 2 ** 20)).any()
    assert [by_name[n].n_vars for n in ("vars_12", "vars_300", "vars_700", "no_variables")] == [12, 300, 700, 0]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("algo, inst, dtype", CASES)
def test_single_run_equals_the_one_replica_engine(algo, inst, dtype, seed, lib_path):
    """seed=s goes through mxs_*_create, seeds=[s] through mxs_*_create_replicas: the same states and modifier tables
    bit for bit after 1, 2 and 10 rounds.  The costs: the single run's replica cost IS its eval_cost (the host's
    sum, over the tables as given); the replica engine's is the device's sum of the same items in another order (over
    the tables narrowed to f32 in f32 mode).  Each lies within cost_bound of the exactly rounded sum of its items
    (tests/replica_cost_reference.py: gamma(n - 1) * sum |item| holds for ANY order of the additions), so where both
    sum the same items -- f64, or tables that f32 holds exactly -- they are at most two bounds apart."""
    graph, params, build = make(algo, inst, dtype, lib_path)
    with build(seed=seed) as one, build(seeds=[seed]) as rep:
        assert one.replicas == rep.replicas == 1 and one.seeds == rep.seeds == [seed]
        for n in (1, 1, 8):
            one.run(n), rep.run(n)
            assert one.cycle_count == rep.cycle_count
            assert_same(snapshot(one), snapshot(rep), f"between the two engines after {one.cycle_count} rounds")
            (c1, v1), (cr, vr) = one.replica_costs(INFINITY), rep.replica_costs(INFINITY)
            assert c1.shape == v1.shape == (1,) and (float(c1[0]), int(v1[0])) == one.eval_cost(infinity=INFINITY)
            idx = one.assignment()[0]
            exact, viol, sum_abs, items = reference_cost(graph, Params(dtype="f64"), idx, INFINITY)
            bound = cost_bound(items, sum_abs)
            assert int(v1[0]) == viol == int(vr[0])
            assert abs(float(c1[0]) - exact) <= bound, (float(c1[0]), exact, bound)
            check_replica_costs(rep, [0], INFINITY, cr, vr)
            if dtype == "f64" or (graph.tables.astype(np.float32) == graph.tables).all():
                assert abs(float(c1[0]) - float(cr[0])) <= 2 * bound, (float(c1[0]), float(cr[0]), bound)
        if algo == "mgm2":
            b = one.best(INFINITY)
            assert (b["replica"], b["cost"], b["violations"]) == (0,) + one.eval_cost(infinity=INFINITY)
            np.testing.assert_array_equal(b["idx"], one.assignment()[0])
        else:
            assert one.pool_bytes == rep.pool_bytes     # one pool


@pytest.mark.parametrize("algo", ["mgm2", "gdba"])
def test_a_single_run_keeps_its_refusals(algo, lib_path):
    inst = instances()[0]
    _, _, build = make(algo, inst, "f64", lib_path, seed=1)
    with build() as one:
        for r in (-1, 1):
            with pytest.raises(MaxSumGpuError, match=f"error {MXS_E_INVALID}: replica out of range"):
                one.state(r)
        if algo == "gdba":
            for r in (-1, 1):
                with pytest.raises(MaxSumGpuError, match=f"error {MXS_E_INVALID}: replica out of range"):
                    one.modifiers(0, replica=r)
            with pytest.raises(MaxSumGpuError, match=f"error {MXS_E_STATE}: gdba: the best state is tracked by the replica engine"):
                one.track_best(1)
            for r in (-1, 0, 7):
                with pytest.raises(MaxSumGpuError, match=f"error {MXS_E_STATE}: mxs_gdba_get_best before mxs_gdba_track_best"):
                    one.best(r)
    if algo == "gdba":      # the budget refusal of a single run names no replicas
        sparse = G.random_coloring(20, avg_degree=1, seed=1)
        with GdbaEngine(sparse, Params(), increase_mode="C", lib_path=lib_path) as e:
            need = e.pool_bytes
        assert need > 0
        with GdbaEngine(sparse, Params(), increase_mode="C", pool_budget=need, lib_path=lib_path) as e:
            assert e.pool_bytes == need
        with pytest.raises(MaxSumGpuError, match=f"error {MXS_E_INVALID}: gdba: the modifier tables take {need} bytes, "
                                                 f"more than the budget of {need - 1}$"):
            GdbaEngine(sparse, Params(), increase_mode="C", pool_budget=need - 1, lib_path=lib_path)
