"""The front end pinned: `api.solve_flat` / `api.solve_flat_dpop` on the emulated build return, key for key and bit for
bit, what tests/golden/api_solve_results.json holds -- recorded by tools/record_api_solve.py with the front end as it was
before its solve paths were merged into one --, and refuse what they refused, with the same words."""
import json
import os
import re

import pytest

from api_solve_common import make_instance, run_case

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_solve_results.json")
with open(GOLDEN) as _f:
    CASES = json.load(_f)

REQUIRED = {
    "maxsum", "amaxsum", "dsa", "mgm", "mgm2", "gdba", "dba",
    "maxsum_cost_every", "maxsum_best_every", "maxsum_cost_and_best_every", "maxsum_until_quiescent",
    "dsa_restarts", "dsa_best_every", "dsa_restarts_best_every", "mgm_keyed_restarts", "mgm2_restarts",
    "gdba_best_every", "gdba_restarts_best_every", "dba_restarts_first", "dba_restarts_each", "dpop", "maxsum_unnamed",
}


@pytest.fixture(scope="module")
def emu_lib():
    from emu.build_emu import build
    return build()


def test_the_recorded_cases_are_all_there():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names) and REQUIRED <= set(names)
    by_name = {c["name"]: c for c in CASES}
    # the records say something: a run that fell silent, one that did not, replicas that differ, DBA's two policies
    assert by_name["maxsum_until_quiescent"]["result"]["quiescent"] is True
    assert by_name["maxsum_until_quiescent_loopy"]["result"]["quiescent_cycle"] is None
    assert by_name["dsa_restarts"]["result"]["replica"] != 0
    assert by_name["dba_restarts_first"]["result"]["stop_rounds"] != by_name["dba_restarts_each"]["result"]["stop_rounds"]
    assert list(by_name["maxsum_unnamed"]["result"]["assignment"])[:2] == ["v0", "v1"]
    assert list(by_name["dpop_unnamed"]["result"]["assignment"])[:2] == ["v0", "v1"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_result_is_the_recorded_one(case, emu_lib):
    from pydcop_amd import api
    res = run_case(api, emu_lib, case["instance"], case["fn"], case["objective"], case["cycles"], case["kw"])
    want = case["result"]
    assert sorted(res) == sorted(want)
    for key in want:
        assert res[key] == want[key], key                  # (floats too: exactly)


REFUSALS = [
    # _check_restarts
    (dict(algo="dsa", restarts=0), "restarts must be at least 1 and best_every at least 0"),
    (dict(algo="dsa", best_every=-1), "restarts must be at least 1 and best_every at least 0"),
    (dict(algo="mgm", draws="random"), 'draws must be "fixed" or "keyed"'),
    (dict(algo="dsa", draws="keyed"), 'draws: algo="mgm" only (the other local searches always key their draws on `seed`)'),
    (dict(algo="mgm", restarts=2), 'restarts: algo="dsa", "mgm2" or "dba", algo="mgm" with draws="keyed", or algo="gdba" '
                                   'with best_every >= 1'),
    (dict(algo="gdba", restarts=2), 'or algo="gdba" with best_every >= 1'),
    (dict(algo="maxsum", restarts=2), 'restarts: algo="dsa", "mgm2" or "dba"'),
    (dict(algo="amaxsum", restarts=2), 'restarts: algo="dsa", "mgm2" or "dba"'),
    (dict(algo="dba", restarts=2, dba_stop="last"), 'dba_stop must be "first" or "each"'),
    (dict(algo="mgm", best_every=1), 'best_every: algo="dsa", "gdba" or "maxsum" only'),
    (dict(algo="mgm2", restarts=2, best_every=1), 'best_every: algo="dsa", "gdba" or "maxsum" only'),
    (dict(algo="dba", best_every=1), 'best_every: algo="dsa", "gdba" or "maxsum" only'),
    (dict(algo="amaxsum", best_every=1), 'best_every: algo="dsa", "gdba" or "maxsum" only'),
    # _check_maxsum_tracking
    (dict(cost_every=4, best_every=1), "maxsum: cost_every and best_every are one evaluation period: give one, or the same value"),
    (dict(best_every=1, devices=2), "best_every: maxsum on one device only (a shard's cost is partial)"),
    # _check_until_quiescent
    (dict(until_quiescent=-1), "until_quiescent must be at least 0"),
    (dict(algo="amaxsum", until_quiescent=1), 'until_quiescent: algo="maxsum" only (amaxsum ends by itself, the others have no send rule)'),
    (dict(algo="dsa", until_quiescent=1), 'until_quiescent: algo="maxsum" only'),
    (dict(until_quiescent=1, devices=2), "until_quiescent: maxsum on one device only (a shard sees its own edges only)"),
    # _engine_for
    (dict(algo="dsa", devices=2), "devices > 1: synchronous Max-Sum only"),
    (dict(algo="amaxsum", devices=2), "devices > 1: synchronous Max-Sum only"),
    (dict(algo="dpop"), "(DPOP runs no cycles: solve_dcop_dpop / solve_flat_dpop)"),
    (dict(algo="adopt"), "algo must be one of ('maxsum', 'amaxsum', 'dsa', 'mgm', 'mgm2', 'gdba', 'dba')"),
]


@pytest.mark.parametrize("kw, text", REFUSALS, ids=lambda x: "-".join(f"{k}={v}" for k, v in x.items()) if isinstance(x, dict) else "")
def test_refusals_keep_their_words(kw, text, emu_lib):
    from pydcop_amd import api
    g = make_instance(dict(n_vars=40, n_factors=70, seed=65))
    with pytest.raises(ValueError, match=re.escape(text)):
        api.solve_flat(g, "min", 5, lib_path=emu_lib, **kw)
