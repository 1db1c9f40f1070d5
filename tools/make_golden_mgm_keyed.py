"""Record MGM fixtures from the REFERENCE (pydcop/algorithms/mgm.py under keyed draws, tests/mgm_keyed_reference.py):
tests/golden/mgm_keyed/<case>.npz = the instance, the Params kwargs, the seed, the number of rounds and what the
reference's own computations hold after them: values and costs.  Variable costs sit on a binary grid, so that the one
order the reference leaves to PYTHONHASHSEED cannot change a sum.  Every recorded case draws both ids and moves.  Runs
only where the reference exists:

    python tools/make_golden_mgm_keyed.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def grid(g, seed, scale=64.0, tables=False):
    rng = np.random.default_rng(seed)
    g.var_cost = rng.integers(0, 32, g.var_cost.shape[0]) / scale
    if tables:
        g.tables = np.round(g.tables * 64) / 64
    return g


def cases():
    """(name, instance, Params kwargs, seed, rounds)"""
    from mgm_common import with_init
    from pydcop_amd import generators as G
    return [
        ("coloring_hard_packed", lambda: grid(G.random_coloring(45, seed=31, variant="hard"), 31, 2.0 ** 30), {"mode": "min"}, 5, 8),
        ("mixed_arity3_max", lambda: grid(G.random_mixed(24, 36, seed=25, float_tables=False), 25), {"mode": "max"}, 3, 6),
        ("ising_unaries", lambda: grid(G.ising_grid(5, 6, seed=26), 26, tables=True), {"mode": "min"}, 7, 6),
        ("meeting_d6", lambda: grid(G.meeting_like(10, dom=6, seed=28), 28), {"mode": "max"}, 2, 6),
        ("coloring_init", lambda: with_init(grid(G.random_coloring(40, seed=23), 23), 23), {"mode": "min"}, 11, 6),
    ]


def main():
    from mgm_keyed_oracle import OracleMgmKeyed
    from mgm_keyed_reference import reference_state
    from oracle import ref_harness
    from pydcop_amd.graph import Params
    if not ref_harness.reference_available():
        raise SystemExit("the reference is not on this machine")
    out_dir = os.path.join(ROOT, "tests", "golden", "mgm_keyed")
    os.makedirs(out_dir, exist_ok=True)
    for name, make, kw, seed, rounds in cases():
        g = make()
        assert g.n_vars <= 60, name
        ref, cycles, _ = reference_state(g, kw["mode"], seed, rounds)
        start = OracleMgmKeyed(g, Params(**kw), draws="keyed", seed=seed).state()["idx"]
        assert cycles and (ref["idx"] != start).any(), name           # draws of id 11 were made, variables moved
        meta = {"kwargs": kw, "seed": seed, "rounds": rounds, "var_names": g.var_names}
        arrays = dict(dom_size=g.dom_size, var_cost=g.var_cost, factor_rowptr=g.factor_rowptr, edge_var=g.edge_var,
                      table_off=g.table_off, tables=g.tables, var_rowptr=g.var_rowptr, var_edges=g.var_edges,
                      ref_idx=ref["idx"], ref_cost=ref["cost"],
                      meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8))
        if g.init_idx is not None:
            arrays["init_idx"] = g.init_idx
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
