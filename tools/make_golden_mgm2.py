"""Record MGM-2 fixtures from the REFERENCE (pydcop/algorithms/mgm2.py under keyed draws,
tests/mgm2_reference.py): tests/golden/mgm2/<case>.npz = the instance, the parameters and, after T rounds,
the values and held costs of the reference's own computations.  Runs only where the reference exists:

    python tools/make_golden_mgm2.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

ROUNDS = 8


def main():
    from mgm2_common import mgm2_cases
    from mgm2_reference import run_reference_mgm2
    from oracle import ref_harness
    if not ref_harness.reference_available():
        raise SystemExit("the reference is not on this machine")
    out_dir = os.path.join(ROOT, "tests", "golden", "mgm2")
    os.makedirs(out_dir, exist_ok=True)
    for name, make, pkw, kw in mgm2_cases(k=2):
        g = make()
        mode = pkw.get("mode", "min")
        dcop, _ = ref_harness.flat_to_dcop(g, mode)
        vals, costs, _ = run_reference_mgm2(dcop, ROUNDS, var_index={n: i for i, n in enumerate(g.var_names)}, **kw)
        doms = g.domains or [list(range(int(d))) for d in g.dom_size]
        ref_idx = np.array([doms[i].index(vals[n]) for i, n in enumerate(g.var_names)], dtype=np.int32)
        ref_cost = np.array([np.nan if costs[n] is None else float(costs[n]) for n in g.var_names])
        meta = {"mode": mode, "rounds": ROUNDS, "mgm2": kw, "var_names": g.var_names}
        arrays = dict(dom_size=g.dom_size, var_cost=g.var_cost, factor_rowptr=g.factor_rowptr, edge_var=g.edge_var,
                      table_off=g.table_off, tables=g.tables, var_rowptr=g.var_rowptr, var_edges=g.var_edges,
                      ref_idx=ref_idx, ref_cost=ref_cost, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8))
        if g.init_idx is not None:
            arrays["init_idx"] = g.init_idx
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
