"""Record DBA fixtures from the REFERENCE (pydcop/algorithms/dba.py under keyed draws, tests/dba_reference.py):
tests/golden/dba/<case>.npz = the instance, the parameters and what the reference's own computations hold after
T rounds or at their stop: values, held costs, evals, improvements, new values, termination counters, consistent
flags and every weight, with the numbers of moves and weight increases, the stop round and the violations left.
Runs only where the reference exists:

    python tools/make_golden_dba.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    from dba_common import ROUNDS, STATE_KEYS, count_violations, dba_cases
    from dba_reference import reference_state
    from oracle import ref_harness
    if not ref_harness.reference_available():
        raise SystemExit("the reference is not on this machine")
    out_dir = os.path.join(ROOT, "tests", "golden", "dba")
    os.makedirs(out_dir, exist_ok=True)
    for name, make, kw in dba_cases():
        g = make()
        ref, weights, info = reference_state(g, kw, ROUNDS)
        info["increases"] = int((weights - 1).sum())
        info["violations"] = count_violations(g, ref["idx"], kw["infinity"])
        meta = {"rounds": ROUNDS, "dba": kw, "var_names": g.var_names, "info": info}
        small = g.tables.astype(np.int32)
        assert np.array_equal(small, g.tables)
        arrays = dict(dom_size=g.dom_size, var_cost=g.var_cost, factor_rowptr=g.factor_rowptr, edge_var=g.edge_var,
                      table_off=g.table_off, tables=small, var_rowptr=g.var_rowptr, var_edges=g.var_edges,
                      ref_weights=weights, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8),
                      **{"ref_" + k: ref[k] for k in STATE_KEYS})
        if g.init_idx is not None:
            arrays["init_idx"] = g.init_idx
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path), info)


if __name__ == "__main__":
    main()
