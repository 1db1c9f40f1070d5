"""MGM-2: the cases and the engine-vs-oracle comparison shared by the emulated (CPU) and the GPU tests."""
import numpy as np

from mgm_common import repeated_pairs_and_unaries, shuffled_names, with_init
from pydcop_amd import generators as G
from pydcop_amd.mgm2 import Mgm2Engine


def binary_tables(g):
    """0 / 1 tables: global gains equal to unilateral ones, where `favor` decides"""
    g.tables = g.tables % 2
    return g


def mgm2_cases(k=1):
    """(name, graph factory, Params kwargs, MGM-2 kwargs); k > 1: graphs k times smaller."""
    return [
        ("coloring_unilateral", lambda: G.random_coloring(300 // k, seed=61), {}, dict(seed=1)),
        ("coloring_no", lambda: G.random_coloring(250 // k, seed=62), {}, dict(favor="no", seed=2)),
        ("coloring_hard_ties_coordinated", lambda: shuffled_names(G.random_coloring(200 // k, seed=63, variant="hard"), 63),
         {}, dict(favor="coordinated", seed=3)),
        ("coloring_init_max", lambda: with_init(G.random_coloring(200 // k, seed=64), 64), {"mode": "max"},
         dict(favor="no", seed=4)),
        ("mixed_dom2to5_arity3", lambda: G.random_mixed(120 // k, 200 // k, seed=65), {}, dict(seed=5)),
        ("mixed_int_arity3_max", lambda: with_init(G.random_mixed(90 // k, 140 // k, seed=66, float_tables=False), 66),
         {"mode": "max"}, dict(favor="coordinated", seed=6)),
        ("int_ties_repeated_pairs", lambda: repeated_pairs_and_unaries(200 // k, 67), {}, dict(favor="no", seed=7)),
        ("int_ties_repeated_pairs_max", lambda: with_init(repeated_pairs_and_unaries(150 // k, 68), 68), {"mode": "max"},
         dict(seed=8)),
        ("sparse_isolated_max", lambda: G.random_coloring(200 // k, avg_degree=1, seed=69), {"mode": "max"},
         dict(favor="coordinated", seed=9)),
        ("threshold_0", lambda: G.random_coloring(150 // k, seed=70), {}, dict(threshold=0.0, seed=10)),
        ("threshold_1", lambda: G.random_coloring(150 // k, seed=71), {}, dict(threshold=1.0, seed=11)),
        ("binary_tables_coordinated", lambda: binary_tables(G.random_coloring(100, seed=74)), {},
         dict(favor="coordinated", threshold=0.6, seed=74)),
        ("binary_tables_no", lambda: binary_tables(G.random_coloring(100, seed=74)), {},
         dict(favor="no", threshold=0.6, seed=74)),
        ("meeting_d6_max", lambda: G.meeting_like(40, dom=6, seed=72), {"mode": "max"}, dict(threshold=0.7, seed=12)),
    ]


def compare_mgm2(oracle_cls, graph, params, kw, lib_path=None, steps=(0, 1, 1, 3, 10)):
    """Round-by-round state (values, held costs, has_cost) bit for bit, and the solution cost."""
    eng = Mgm2Engine(graph, params, lib_path=lib_path, **kw)
    ora = oracle_cls(graph, params, **kw)
    done = 0
    for n in steps:
        eng.run(n), ora.run(n)
        done += n
        assert eng.cycle_count == ora.cycle_count == done
        se, so = eng.state(), ora.state()
        for key in ("idx", "has_cost", "cost"):
            np.testing.assert_array_equal(se[key], so[key], err_msg=f"{key} after {done} rounds")
        ce, co = eng.eval_cost(), ora.eval_cost()
        assert ce[1] == co[1] and abs(ce[0] - co[0]) <= 1e-9 * max(1.0, abs(co[0]))
    eng.reset(), ora.reset()
    eng.run(2), ora.run(2)
    np.testing.assert_array_equal(eng.state()["idx"], ora.state()["idx"])
    np.testing.assert_array_equal(eng.state()["cost"], ora.state()["cost"])
    eng.close(), ora.close()


def mgm2_golden_files():
    import glob
    import os
    return sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mgm2", "*.npz")))


def load_mgm2_golden(path):
    """tools/make_golden_mgm2.py -> (FlatGraph, Params kwargs, MGM-2 kwargs, rounds, ref_idx, ref_cost
    (NaN: the computation still holds None))"""
    import json
    from pydcop_amd.graph import FlatGraph
    z = np.load(path)
    meta = json.loads(bytes(z["meta"]).decode())
    g = FlatGraph(dom_size=z["dom_size"], var_cost=z["var_cost"], factor_rowptr=z["factor_rowptr"],
                  edge_var=z["edge_var"], table_off=z["table_off"], tables=z["tables"],
                  var_rowptr=z["var_rowptr"], var_edges=z["var_edges"],
                  init_idx=z["init_idx"] if "init_idx" in z.files else None)
    g.var_names = meta["var_names"]
    return g.validate(), {"mode": meta["mode"]}, meta["mgm2"], meta["rounds"], z["ref_idx"], z["ref_cost"]


def check_golden(state, ref_idx, ref_cost):
    np.testing.assert_array_equal(state["idx"], ref_idx)
    held = ~np.isnan(ref_cost)
    np.testing.assert_array_equal(state["has_cost"].astype(bool), held)
    np.testing.assert_array_equal(state["cost"][held], ref_cost[held])
