"""Pins tests/mgm2_oracle.py against the REAL reference: the reference's own Mgm2Computation objects
(pydcop/algorithms/mgm2.py) run for exactly R rounds under keyed draws by
tests/mgm2_reference.run_reference_mgm2 -- selected values and held costs (`current_cost`), bit for
bit.  Where the reference is on the machine (oracle/stage_reference.locate())."""
import os

import numpy as np
import pytest

from mgm2_common import mgm2_cases
from oracle import ref_harness
from pydcop_amd.graph import Params

pytestmark = pytest.mark.skipif(not ref_harness.reference_available(), reason="reference tree not present")


def check_against_reference(g, mode, kw, rounds):
    from mgm2_oracle import OracleMgm2
    from mgm2_reference import run_reference_mgm2
    dcop, _ = ref_harness.flat_to_dcop(g, mode)
    index = {n: i for i, n in enumerate(g.var_names)}
    vals, costs, comps = run_reference_mgm2(dcop, rounds, var_index=index, **kw)
    o = OracleMgm2(g, Params(mode=mode), **kw)
    o.run(rounds)
    st = o.state()
    doms = g.domains or [list(range(int(d))) for d in g.dom_size]
    ref_idx = np.array([doms[i].index(vals[n]) for i, n in enumerate(g.var_names)])
    np.testing.assert_array_equal(st["idx"], ref_idx)
    for i, n in enumerate(g.var_names):
        if costs[n] is None:
            assert not st["has_cost"][i], n
        else:
            assert st["has_cost"][i] and st["cost"][i] == costs[n], (n, st["cost"][i], costs[n])
    viol, cost = dcop.solution_cost(vals, float("inf"))
    ocost, oviol = o.eval_cost()
    assert oviol == viol and ocost == pytest.approx(cost, rel=1e-12, abs=1e-9)
    assert all(c.cycle_count == rounds + 1 for c in comps.values() if c._neighbors)
    return st


@pytest.mark.parametrize("case", mgm2_cases(k=2), ids=lambda c: c[0])
@pytest.mark.parametrize("rounds", [0, 1, 3, 8])
def test_mgm2_oracle_equals_reference(case, rounds):
    name, make, pkw, kw = case
    check_against_reference(make(), pkw.get("mode", "min"), kw, rounds)


def test_mgm2_oracle_moves():
    """Not a fixed point: the cases do move (offers accepted, coordinated moves made)."""
    from mgm2_oracle import OracleMgm2
    from pydcop_amd import generators as G
    g = G.random_coloring(150, seed=3)
    o = OracleMgm2(g, Params(), threshold=1.0 - 1e-9, seed=3)
    start = o.eval_cost()[0]
    o.run(10)
    assert o.eval_cost()[0] < 0.8 * start


@pytest.mark.parametrize("instance", ["graph_coloring1.yaml", "graph_coloring_tuto.yaml",
                                      "graph_coloring_3agts_10vars.yaml", "graph_coloring_10_4_15_0.1.yml",
                                      "graph_coloring_tuto_max.yaml"])
@pytest.mark.parametrize("favor", ["unilateral", "no", "coordinated"])
def test_mgm2_oracle_equals_reference_on_yaml(instance, favor):
    """The reference's own graph-colouring instances, compiled as the mgm2_gpu plug-in compiles them."""
    from mgm2_oracle import OracleMgm2
    from mgm2_reference import run_reference_mgm2
    ref_harness.install_shims()
    from pydcop.dcop.yamldcop import load_dcop_from_file
    from pydcop_amd.algorithms.mgm2_gpu import compile_dcop_for_local_search
    path = os.path.join(ref_harness.REFERENCE_ROOT, "tests", "instances", instance)
    dcop = load_dcop_from_file([path])
    g = compile_dcop_for_local_search(dcop)
    index = {n: i for i, n in enumerate(g.var_names)}
    for rounds in (1, 4, 9):
        vals, costs, _ = run_reference_mgm2(load_dcop_from_file([path]), rounds, favor=favor, seed=5, var_index=index)
        o = OracleMgm2(g, Params(mode=dcop.objective), favor=favor, seed=5)
        o.run(rounds)
        idx = o.state()["idx"]
        assert {n: g.domains[i][idx[i]] for i, n in enumerate(g.var_names)} == vals
        for i, n in enumerate(g.var_names):
            assert costs[n] is None or o.state()["cost"][i] == costs[n]


def _fuzz_seeds():
    from fuzz_common import mgm2_instance, small_seeds
    return small_seeds(mgm2_instance)


@pytest.mark.parametrize("seed", _fuzz_seeds())
def test_mgm2_oracle_equals_reference_on_random_instances(seed):
    """the small end of the sweep of tests/fuzz_common.py: unequal neighbour domains, every favor / threshold"""
    from fuzz_common import mgm2_instance
    g, p, kw = mgm2_instance(seed)
    for rounds in (1, 4, 10):
        check_against_reference(g, p.mode, kw, rounds)
