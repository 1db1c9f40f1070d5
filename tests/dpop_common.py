"""DPOP: the cases and the engine-vs-oracle comparison shared by the emulated (CPU) and the GPU tests."""
import glob
import json
import os

import numpy as np

from mgm_common import repeated_pairs_and_unaries, shuffled_names
from pydcop_amd import generators as G
from pydcop_amd.dpop import DpopEngine
from pydcop_amd.graph import FlatGraph, Params

HERE = os.path.dirname(os.path.abspath(__file__))
FUSE = (-1, 0, 2 ** 31 - 1)      # the built-in cap, one launch per level, fuse whatever is there


def int_ties(g, levels=3):
    """Integer tables and variable costs on a few levels: ties everywhere, the FIRST optimum decides"""
    rng = np.random.default_rng(int(g.n_vars))
    g.tables = rng.integers(0, levels, g.tables.shape[0]).astype(np.float64)
    g.var_cost = rng.integers(0, 2, g.var_cost.shape[0]).astype(np.float64)
    return g


def dpop_cases():
    """(name, graph factory, Params kwargs): every one at or below about 10 000 UTIL entries in all (the
    reference's join is a Python loop over assignment dictionaries)."""
    return [
        ("ising_3x10", lambda: G.ising_grid(3, 10, seed=1), {}),
        ("ising_4x12", lambda: G.ising_grid(4, 12, seed=1), {}),
        ("ising_3x10_max", lambda: G.ising_grid(3, 10, seed=2), {"mode": "max"}),
        ("coloring_30", lambda: G.random_coloring(30, avg_degree=2, seed=5), {}),
        ("coloring_30_max", lambda: G.random_coloring(30, avg_degree=2, seed=6), {"mode": "max"}),
        ("coloring_hard_shuffled_names", lambda: shuffled_names(G.random_coloring(30, avg_degree=2, seed=7, variant="hard"), 7), {}),
        ("forest_isolated", lambda: G.random_coloring(40, avg_degree=1, seed=8), {}),
        ("forest_isolated_max", lambda: G.random_coloring(40, avg_degree=1, seed=9), {"mode": "max"}),
        ("mixed_20_24", lambda: G.random_mixed(20, 24, seed=10), {}),
        ("mixed_int_max", lambda: G.random_mixed(16, 18, seed=11, float_tables=False), {"mode": "max"}),
        ("int_ties_coloring", lambda: int_ties(G.random_coloring(30, avg_degree=2, seed=12)), {}),
        ("int_ties_coloring_max", lambda: int_ties(G.random_coloring(30, avg_degree=2, seed=13), 2), {"mode": "max"}),
        ("repeated_pairs_unaries", lambda: repeated_pairs_and_unaries(24, 14), {}),
        ("meeting_8_d4", lambda: G.meeting_like(8, dom=4, seed=15), {"mode": "max"}),
    ]


def compare_dpop(oracle_cls, graph, params, lib_path=None, fuse=FUSE, all_utils=True, tree=None):
    """idx, cost, every UTIL (in the oracle's = the reference's dimension order) and stats(), bit for bit; the
    fused and the per-level launch plans give the same bits."""
    ora = oracle_cls(graph, params, tree=tree).solve()
    so, sto = ora.state(), ora.stats()
    word = 4 if params.dtype == "f32" else 8
    for f in fuse:
        with DpopEngine(graph, params, tree=tree, fuse_entries=f, lib_path=lib_path) as eng:
            eng.solve()
            se = eng.state()
            print(f"fuse_entries={f}: {eng.stats()}")
            np.testing.assert_array_equal(se["idx"], so["idx"], err_msg=f"idx, fuse_entries={f}")
            np.testing.assert_array_equal(se["cost"], so["cost"], err_msg=f"cost, fuse_entries={f}")
            ste = eng.stats()
            for k, x in sto.items():
                assert ste[k] == x, (k, ste[k], x)
            assert ste["bytes"] == ste["total_entries"] * word
            if f == 0:
                assert ste["launches_value"] == ste["depth"] + 1
            elif f == FUSE[-1]:
                assert ste["launches_util"] <= 1 and ste["launches_value"] <= 1
            wanted = sorted(ora.util, key=lambda v: -ora.util[v][1].size)
            for v in wanted if all_utils else wanted[:1] + [v for v in wanted if ora.parent[ora.parent[v]] < 0]:
                dims, table = eng.util(v)
                odims, otable = ora.util[v]
                assert list(dims) == list(odims), (v, dims, odims)
                np.testing.assert_array_equal(table, otable.astype(np.float64), err_msg=f"UTIL of {v}, fuse_entries={f}")
            assert abs(eng.eval_cost()[0] - ora.eval_cost()) <= 1e-9 * max(1.0, abs(ora.eval_cost()))
    return ora


def dpop_golden_files():
    return sorted(glob.glob(os.path.join(HERE, "golden", "dpop", "*.npz")))


def load_dpop_golden(path):
    """tools/make_golden_dpop.py -> (FlatGraph, Params kwargs, tree, ref_idx, ref_cost, {var: (dims, table)}):
    what the reference's own DpopAlgo objects selected, reported and sent."""
    z = np.load(path)
    meta = json.loads(bytes(z["meta"]).decode())
    g = FlatGraph(dom_size=z["dom_size"], var_cost=z["var_cost"], factor_rowptr=z["factor_rowptr"],
                  edge_var=z["edge_var"], table_off=z["table_off"], tables=z["tables"],
                  var_rowptr=z["var_rowptr"], var_edges=z["var_edges"])
    g.var_names = meta["var_names"]
    utils = {}
    for i, v in enumerate(z["util_var"]):
        dims = z["util_dims"][z["util_dims_off"][i]:z["util_dims_off"][i + 1]]
        data = z["util_data"][z["util_data_off"][i]:z["util_data_off"][i + 1]]
        utils[int(v)] = (dims, data.reshape([int(g.dom_size[u]) for u in dims]))
    tree = (z["parent"], z["child_rowptr"], z["child_idx"])
    return g.validate(), {"mode": meta["mode"]}, tree, z["ref_idx"], z["ref_cost"], utils


def check_golden(solver, ref_idx, ref_cost, utils):
    """`solver`: a solved DpopEngine or OracleDpop (f64)"""
    st = solver.state()
    np.testing.assert_array_equal(st["idx"], ref_idx)
    np.testing.assert_array_equal(st["cost"], ref_cost)
    for v, (dims, table) in utils.items():
        d, t = solver.util(v) if callable(solver.util) else solver.util[v]
        assert list(d) == list(dims), v
        np.testing.assert_array_equal(np.asarray(t, dtype=np.float64), table, err_msg=f"UTIL of {v}")
