"""What tools/record_api_solve.py (the recorder of tests/golden/api_solve_results.json) and tests/test_api_solve_golden.py
(its replay) share: how a recorded case becomes an instance and a call."""
import json

from pydcop_amd import generators as G


def make_instance(spec):
    """the kwargs of generators.random_mixed; `violated_from` = t: tables of 1000 where the entry is >= t, else 0"""
    spec = dict(spec)
    t = spec.pop("violated_from", None)
    g = G.random_mixed(**spec)
    if t is not None:
        g.tables = 1000.0 * (g.tables >= t)
    return g


def run_case(api, lib_path, instance, fn, objective, cycles, kw):
    """the call the recorder and the test both make -> the result as JSON holds it (tuples are lists, numpy scalars
    plain numbers)"""
    args = (objective,) if cycles is None else (objective, cycles)
    res = getattr(api, fn)(make_instance(instance), *args, infinity=10000.0, lib_path=lib_path, **kw)
    return json.loads(json.dumps(res, default=lambda x: x.item()))
