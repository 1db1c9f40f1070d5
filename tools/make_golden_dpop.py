"""Record DPOP fixtures from the REFERENCE (pydcop/algorithms/dpop.py on pseudotree.build_computation_graph,
tests/dpop_reference.py): tests/golden/dpop/<case>.npz = the instance, the reference's tree, the values its
DpopAlgo objects selected, the costs they reported and the UTIL tables they sent, with their dimension lists
(recorded data only).  UTILs above KEEP entries are left out to keep a fixture at tens of KB: the narrow,
root-ward ones remain.  Runs only where the reference exists:

    python tools/make_golden_dpop.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

KEEP = 1024


def main():
    from dpop_common import dpop_cases
    from dpop_reference import run_reference_dpop
    from oracle import ref_harness
    from pydcop_amd import generators as G
    from pydcop_amd.dpop import pack_tree
    if not ref_harness.reference_available():
        raise SystemExit("the reference is not on this machine")
    out_dir = os.path.join(ROOT, "tests", "golden", "dpop")
    os.makedirs(out_dir, exist_ok=True)
    cases = [c for c in dpop_cases() if c[0] != "ising_4x12"] + [
        ("coloring_40_deg3", lambda: G.random_coloring(40, avg_degree=3, seed=3), {})]
    for name, make, pkw in cases:
        g = make()
        mode = pkw.get("mode", "min")
        dcop, _ = ref_harness.flat_to_dcop(g, mode)
        vals, costs, utils, rel = run_reference_dpop(dcop)
        names = g.var_names
        index = {n: i for i, n in enumerate(names)}
        doms = g.domains or [list(range(int(d))) for d in g.dom_size]
        parent = [-1 if rel[n][0] is None else index[rel[n][0]] for n in names]
        children = [[index[c] for c in rel[n][2]] for n in names]
        parent, crow, cidx = pack_tree(parent, children)
        kept = sorted(index[n] for n, (_, t) in utils.items() if t.size <= KEEP)
        dims = [np.array([index[u] for u in utils[names[v]][0]], dtype=np.int32) for v in kept]
        data = [utils[names[v]][1].reshape(-1) for v in kept]
        off = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)
        meta = {"mode": mode, "var_names": names, "total_entries": int(sum(t.size for _, t in utils.values()))}
        arrays = dict(dom_size=g.dom_size, var_cost=g.var_cost, factor_rowptr=g.factor_rowptr, edge_var=g.edge_var,
                      table_off=g.table_off, tables=g.tables, var_rowptr=g.var_rowptr, var_edges=g.var_edges,
                      parent=parent, child_rowptr=crow, child_idx=cidx,
                      ref_idx=np.array([doms[i].index(vals[n]) for i, n in enumerate(names)], dtype=np.int32),
                      ref_cost=np.array([float(costs[n]) for n in names]),
                      util_var=np.array(kept, dtype=np.int32), util_dims=cat(dims, np.int32), util_dims_off=off(dims),
                      util_data=cat(data, np.float64), util_data_off=off(data),
                      meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8))
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path), meta["total_entries"])


if __name__ == "__main__":
    main()
