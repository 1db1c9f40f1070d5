"""Record what `api.solve_flat` / `api.solve_flat_dpop` return on the emulated build, for tests/test_api_solve_golden.py:
tests/golden/api_solve_results.json = a list of {name, instance (the kwargs of generators.random_mixed; `violated_from`
= t turns the tables into 1000 where the entry is >= t and 0 elsewhere), fn, objective, cycles, kw, result}.  The test
replays every entry and compares the whole result dictionary, floats exactly (the emulated build is deterministic, JSON
round-trips doubles), so the file pins the front end: record it with the front end that is to be matched, i.e. BEFORE
changing pydcop_amd/api.py (or from a checkout of the commit to match), never after.

    python tools/record_api_solve.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

FLOAT = dict(n_vars=40, n_factors=70, seed=65)                                   # real tables, variable costs
INT = dict(n_vars=40, n_factors=70, seed=65, float_tables=False, unary_noise=0)  # integers 0..9: every cost is exact
UNNAMED = dict(FLOAT, names=False)                                               # no var_names: the v{i} fallback
TREE = dict(n_vars=20, n_factors=24, seed=21, float_tables=False)                # (a second, smaller tree for DPOP)
SPARSE = dict(n_vars=40, n_factors=40, seed=65)                                  # Max-Sum falls silent (cycle 43)
HARD = dict(INT, violated_from=9)                                                # 0 / 1000 tables: DBA's constraints
HARDER = dict(INT, violated_from=6)                                              # (no run stops within 30 rounds)
DBA = dict(dba_infinity=1000, max_distance=3)


def cases():
    """(name, instance, fn, objective, cycles, kw)"""
    flat = lambda name, inst, cycles, **kw: (name, inst, "solve_flat", "min", cycles, kw)    # noqa: E731
    return [
        # every algorithm with its defaults
        flat("maxsum", FLOAT, 20),
        flat("amaxsum", FLOAT, 20, algo="amaxsum"),
        flat("dsa", FLOAT, 20, algo="dsa"),
        flat("mgm", FLOAT, 20, algo="mgm"),
        flat("mgm2", FLOAT, 20, algo="mgm2"),
        flat("gdba", INT, 20, algo="gdba"),
        flat("dba", HARD, 40, algo="dba", **DBA),
        ("maxsum_max", FLOAT, "solve_flat", "max", 20, {}),
        flat("amaxsum_cost_every", FLOAT, 20, algo="amaxsum", cost_every=6),
        flat("dsa_cost_every", FLOAT, 20, algo="dsa", cost_every=6, seed=3),
        # Max-Sum's device-side tracking and end condition
        flat("maxsum_cost_every", FLOAT, 22, cost_every=4),
        flat("maxsum_best_every", FLOAT, 22, best_every=1),
        flat("maxsum_cost_and_best_every", FLOAT, 22, cost_every=4, best_every=4),
        flat("maxsum_until_quiescent", SPARSE, 300, until_quiescent=1),
        flat("maxsum_until_quiescent_loopy", FLOAT, 100, until_quiescent=1),
        flat("maxsum_until_quiescent_capped", FLOAT, 10, until_quiescent=3, cost_every=4),
        flat("maxsum_until_quiescent_best_every", SPARSE, 300, until_quiescent=2, best_every=5, cost_every=5),
        # replicas and records
        flat("dsa_restarts", FLOAT, 20, algo="dsa", seed=5, restarts=4),
        flat("dsa_best_every", FLOAT, 20, algo="dsa", seed=5, best_every=1),
        flat("dsa_restarts_best_every", FLOAT, 20, algo="dsa", seed=5, restarts=4, best_every=1, variant="A",
             probability=0.5, cost_every=5),
        flat("mgm_keyed", FLOAT, 20, algo="mgm", draws="keyed", seed=5),
        flat("mgm_keyed_restarts", FLOAT, 20, algo="mgm", draws="keyed", seed=5, restarts=4),
        flat("mgm2_restarts", FLOAT, 20, algo="mgm2", seed=5, restarts=4, favor="coordinated", threshold=0.4),
        flat("gdba_best_every", INT, 30, algo="gdba", seed=5, best_every=1, modifier="M", violation="NM", increase_mode="T"),
        flat("gdba_restarts_best_every", INT, 30, algo="gdba", seed=5, restarts=4, best_every=1, modifier="M",
             violation="NM", increase_mode="T"),
        flat("dba_restarts_first", HARD, 60, algo="dba", seed=5, restarts=4, **DBA),
        flat("dba_restarts_each", HARD, 60, algo="dba", seed=5, restarts=4, dba_stop="each", **DBA),
        flat("dba_restarts_running", HARDER, 30, algo="dba", seed=5, restarts=4, dba_stop="each", **DBA),
        # no names
        flat("maxsum_unnamed", UNNAMED, 20),
        flat("dsa_unnamed_restarts", UNNAMED, 20, algo="dsa", seed=5, restarts=4),
        # DPOP
        ("dpop", FLOAT, "solve_flat_dpop", "min", None, {}),
        ("dpop_small", TREE, "solve_flat_dpop", "min", None, {}),
        ("dpop_max_f32", TREE, "solve_flat_dpop", "max", None, {"precision": "f32"}),
        ("dpop_unnamed", dict(TREE, names=False), "solve_flat_dpop", "min", None, {}),
    ]


def main(out=os.path.join(ROOT, "tests", "golden", "api_solve_results.json")):
    from api_solve_common import run_case
    from emu.build_emu import build
    from pydcop_amd import api, engine
    lib_path = build()
    engine.register_test_engine(lib_path)
    records = [dict(name=name, instance=inst, fn=fn, objective=objective, cycles=cycles, kw=kw,
                    result=run_case(api, lib_path, inst, fn, objective, cycles, kw))
               for name, inst, fn, objective, cycles, kw in cases()]
    with open(out, "w") as f:
        json.dump(records, f, indent=1, sort_keys=True)
        f.write("\n")
    print(out, os.path.getsize(out), "bytes,", len(records), "cases from", api.__file__)


if __name__ == "__main__":
    main(*sys.argv[1:])
