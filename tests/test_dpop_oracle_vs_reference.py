"""Pins tests/dpop_oracle.py and the pseudo-tree builders against the REAL reference: the reference's own
DpopAlgo objects on the reference's own pseudo-tree (tests/dpop_reference.py), UTIL messages delivered in
children-list order -- values, reported costs and EVERY UTIL table bit for bit; parent, children order,
pseudo-parents and pseudo-children of `build_pseudotree` / `pseudotree_fast` equal to
pseudotree.build_computation_graph.  Where the reference is on the machine (oracle/stage_reference.locate())."""
import os

import numpy as np
import pytest

from dpop_common import dpop_cases
from oracle import ref_harness
from pydcop_amd.graph import Params

pytestmark = pytest.mark.skipif(not ref_harness.reference_available(), reason="reference tree not present")

YAML = ["graph_coloring1.yaml", "graph_coloring_tuto.yaml", "graph_coloring_tuto_max.yaml",
        "graph_coloring_3agts_10vars.yaml", "graph_coloring_10_4_15_0.1.yml", "secp_simple1.yaml"]


def same_tree(g, rel):
    """build_pseudotree(g) against the reference's relations by name"""
    from pydcop_amd.dpop import dfs_pseudotree, neighbor_lists
    names = g.var_names
    _, parent, children, pps, pcs = dfs_pseudotree(neighbor_lists(g))
    for i, n in enumerate(names):
        p, pp, ch, pc = rel[n]
        assert (None if parent[i] < 0 else names[parent[i]]) == p, n
        assert [names[c] for c in children[i]] == ch, n
        assert [names[c] for c in pps[i]] == pp, n
        assert [names[c] for c in pcs[i]] == pc, n


def check_against_reference(g, mode):
    from dpop_oracle import OracleDpop
    from dpop_reference import run_reference_dpop
    dcop, _ = ref_harness.flat_to_dcop(g, mode)
    vals, costs, utils, rel = run_reference_dpop(dcop)
    same_tree(g, rel)
    o = OracleDpop(g, Params(mode=mode)).solve()
    doms = g.domains or [list(range(int(d))) for d in g.dom_size]
    index = {n: i for i, n in enumerate(g.var_names)}
    st = o.state()
    np.testing.assert_array_equal(st["idx"], [doms[i].index(vals[n]) for i, n in enumerate(g.var_names)])
    np.testing.assert_array_equal(st["cost"], [float(costs[n]) for n in g.var_names])
    assert set(utils) == {g.var_names[v] for v in o.util}
    for n, (dims, table) in utils.items():
        odims, otable = o.util[index[n]]
        assert [g.var_names[u] for u in odims] == dims, n
        np.testing.assert_array_equal(otable, table, err_msg=f"UTIL of {n}")
    viol, cost = dcop.solution_cost(vals, float("inf"))
    assert viol == 0 and o.eval_cost() == pytest.approx(cost, rel=1e-12, abs=1e-9)
    return vals, costs, utils, rel, o


@pytest.mark.parametrize("case", dpop_cases(), ids=lambda c: c[0])
def test_dpop_oracle_equals_reference(case):
    name, make, pkw = case
    g = make()
    *_, o = check_against_reference(g, pkw.get("mode", "min"))
    assert o.stats()["total_entries"] <= 12_000     # (the reference's join is a Python loop)


@pytest.mark.parametrize("case", dpop_cases(), ids=lambda c: c[0])
def test_pseudotree_fast_equals_reference(case):
    """the graph-module twin: a ComputationPseudoTree with equal nodes and links, in the same order"""
    from dpop_reference import reference_tree
    dcop, _ = ref_harness.flat_to_dcop(case[1](), "min")
    _same_graph(dcop, reference_tree(dcop)[0])


def _same_graph(dcop, ref):
    from pydcop_amd import plugin
    plugin.install()
    from pydcop.computations_graph import pseudotree_fast
    fast = pseudotree_fast.build_computation_graph(dcop)
    assert [n.name for n in fast.nodes] == [n.name for n in ref.nodes]
    assert [r.name for r in fast.roots] == [r.name for r in ref.roots]
    for a, b in zip(fast.nodes, ref.nodes):
        assert a == b and a.type == b.type
        assert [c.name for c in a.constraints] == [c.name for c in b.constraints]
        assert [(l.type, l.source, l.target) for l in a.links] == [(l.type, l.source, l.target) for l in b.links]


@pytest.mark.parametrize("instance", YAML)
def test_dpop_oracle_and_trees_equal_reference_on_yaml(instance):
    """The reference's own instances, compiled as the dpop_gpu plug-in compiles them."""
    from dpop_oracle import OracleDpop
    from dpop_reference import reference_tree, run_reference_dpop
    ref_harness.install_shims()
    from pydcop.dcop.yamldcop import load_dcop_from_file
    from pydcop_amd.algorithms.dpop_gpu import compile_pseudotree
    path = os.path.join(ref_harness.REFERENCE_ROOT, "tests", "instances", instance)
    dcop = load_dcop_from_file([path])
    cg, _ = reference_tree(dcop)
    _same_graph(dcop, cg)
    vals, costs, utils, rel = run_reference_dpop(dcop, cg)
    g, tree = compile_pseudotree(cg.nodes)
    o = OracleDpop(g, Params(mode=dcop.objective), tree=tree).solve()
    idx = o.state()["idx"]
    assert {n: g.domains[i][idx[i]] for i, n in enumerate(g.var_names)} == vals
    for i, n in enumerate(g.var_names):
        assert o.state()["cost"][i] == costs[n], n
    for n, (dims, table) in utils.items():
        odims, otable = o.util[g.var_names.index(n)]
        assert [g.var_names[u] for u in odims] == dims
        np.testing.assert_array_equal(otable, table)


def _fuzz_seeds():
    from fuzz_common import dpop_instance, measure_tree, small_seeds
    from pydcop_amd.dpop import build_pseudotree
    # (the reference builds its own tree: the seeds of build_pseudotree's; its join is a Python loop)
    return small_seeds(dpop_instance, n=6, ok=lambda g, p, tree, _: tree is None and measure_tree(g, build_pseudotree(g))[1] <= 12_000)


@pytest.mark.parametrize("seed", _fuzz_seeds())
def test_dpop_oracle_equals_reference_on_random_instances(seed):
    """the small end of the sweep of tests/fuzz_common.py: one-value variables, forests, unequal domains"""
    from fuzz_common import dpop_instance
    g, p, _, _ = dpop_instance(seed)
    check_against_reference(g, p.mode)
