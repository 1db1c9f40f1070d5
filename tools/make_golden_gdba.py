"""Record GDBA fixtures from the REFERENCE (pydcop/algorithms/gdba.py under keyed draws,
tests/gdba_reference.py): tests/golden/gdba/<case>.npz = the instance, the parameters and, after T rounds,
what the reference's own computations hold: values, costs, improvements, new values and the modifier tables
of the slots a look-up can reach.  Every recorded case moves and increases.  Runs only where the reference
exists:

    python tools/make_golden_gdba.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    from gdba_common import ROUNDS, gdba_cases
    from gdba_oracle import OracleGdba
    from oracle import ref_harness
    from pydcop_amd.graph import Params
    from gdba_reference import reference_state
    if not ref_harness.reference_available():
        raise SystemExit("the reference is not on this machine")
    out_dir = os.path.join(ROOT, "tests", "golden", "gdba")
    os.makedirs(out_dir, exist_ok=True)
    for name, make, pkw, kw in gdba_cases():
        g = make()
        mode = pkw["mode"]
        ref, mods, moves, _ = reference_state(g, mode, kw, ROUNDS)
        # which slots store a table is a property of the graph (scope = {v} + neighbours(v)); the oracle's
        # plan names them, the recorded entries are the reference's
        plan = OracleGdba(g, Params(mode=mode), **kw)
        base = 0 if kw["modifier"] == "A" else 1
        kept = []
        for s, m in enumerate(mods):
            n = len(plan.modifiers(s))
            if n == 0:
                assert (m == base).all(), (name, s)
                kept.append(m[:0])
            elif kw["increase_mode"] == "T":
                assert (m == m[0]).all(), (name, s)
                kept.append(m[:1])
            else:
                kept.append(m)
        mod = np.concatenate(kept).astype(np.int32) if kept else np.zeros(0, dtype=np.int32)
        mod_off = np.concatenate([[0], np.cumsum([len(m) for m in kept])]).astype(np.int64)
        assert moves > 0 and (mod != base).any(), name
        meta = {"mode": mode, "rounds": ROUNDS, "gdba": kw, "var_names": g.var_names}
        arrays = dict(dom_size=g.dom_size, var_cost=g.var_cost, factor_rowptr=g.factor_rowptr, edge_var=g.edge_var,
                      table_off=g.table_off, tables=g.tables, var_rowptr=g.var_rowptr, var_edges=g.var_edges,
                      ref_idx=ref["idx"], ref_cost=ref["cost"], ref_improve=ref["improve"], ref_new=ref["new"],
                      ref_mod=mod, ref_mod_off=mod_off, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8))
        if g.init_idx is not None:
            arrays["init_idx"] = g.init_idx
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
