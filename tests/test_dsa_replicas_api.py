"""DSA replicas above the engine, on the emulated build: the refusals and the version of C-ABI 2.7, `solve_flat` /
`solve_dcop` / the CLI with `restarts` and `best_every`, and the `dsa_gpu` plug-in behind an unmodified pyDCOP (as
tests/test_dba_plugin.py does for DBA; those need the reference checkout)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import dsa_replicas_common as R
from oracle.stage_reference import locate as _locate_reference
from pydcop_amd import generators as G
from pydcop_amd.dsa import DsaEngine
from pydcop_amd.engine import MaxSumGpuError, load_library
from pydcop_amd.graph import Params

REF = _locate_reference() or ""
needs_pydcop = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "pydcop")),
                                  reason="the pyDCOP reference checkout is not on this machine")
MXS_E_INVALID, MXS_E_STATE = -1, -5


@pytest.fixture(scope="module")
def emu_lib():
    from emu.build_emu import build
    return build()


def test_version_and_refusals(emu_lib):
    lib = load_library(emu_lib)
    assert lib.mxs_version() == 270
    g = G.random_coloring(12, seed=1)
    cg, cp = g.to_c(), Params().to_c()
    seeds = np.arange(4097, dtype=np.uint64)
    for n in (0, 4097, -3):
        h = C.c_void_p()
        rc = lib.mxs_dsa_create_replicas(C.byref(cg), C.byref(cp), 1, 0.7, 0, seeds.ctypes.data, n, 0, C.byref(h))
        assert rc == MXS_E_INVALID and not h.value, n
        assert "replicas" in lib.mxs_last_error().decode()
    h = C.c_void_p()
    assert lib.mxs_dsa_create_replicas(C.byref(cg), C.byref(cp), 1, 0.7, 0, seeds.ctypes.data, 3, 0, C.byref(h)) == 0
    n = C.c_int32(0)
    assert lib.mxs_dsa_replicas(h, C.byref(n)) == 0 and n.value == 3
    idx = np.empty(g.n_vars, dtype=np.int32)
    for r in (-1, 3):
        assert lib.mxs_dsa_get_state_replica(h, r, idx.ctypes.data, None) == MXS_E_INVALID
    for r in (-2, 3):
        assert lib.mxs_dsa_get_best(h, r, None, None, None, None, None) == MXS_E_INVALID
    assert lib.mxs_dsa_get_best(h, -1, None, None, None, None, None) == MXS_E_STATE     # before track_best
    assert lib.mxs_dsa_track_best(h, -1, 1000.0) == MXS_E_INVALID
    assert lib.mxs_dsa_get_best(h, -1, None, None, None, None, None) == MXS_E_STATE     # (a refused call changes nothing)
    assert lib.mxs_dsa_track_best(h, 0, 1000.0) == 0
    assert lib.mxs_dsa_get_best(h, -1, None, None, None, None, None) == 0
    assert lib.mxs_dsa_destroy(h) == 0
    with pytest.raises(MaxSumGpuError, match="replicas"):
        DsaEngine(g, replicas=0, lib_path=emu_lib)
    with pytest.raises(ValueError, match="seeds"):
        DsaEngine(g, replicas=3, seeds=[1, 2], lib_path=emu_lib)


def test_create_is_one_replica(emu_lib):
    """mxs_dsa_create (the binding no longer calls it) is mxs_dsa_create_replicas with one seed"""
    lib = load_library(emu_lib)
    g = G.random_coloring(30, seed=2)
    cg, cp = g.to_c(), Params().to_c()
    h = C.c_void_p()
    assert lib.mxs_dsa_create(C.byref(cg), C.byref(cp), 1, 0.7, 0, 11, 0, C.byref(h)) == 0
    assert lib.mxs_dsa_run(h, 6) == 0
    idx, cost = np.empty(g.n_vars, dtype=np.int32), np.empty(g.n_vars)
    assert lib.mxs_dsa_get_state(h, idx.ctypes.data, cost.ctypes.data) == 0
    lib.mxs_dsa_destroy(h)
    with DsaEngine(g, variant="B", seed=9, replicas=3, lib_path=emu_lib) as e:
        e.run(6)
        np.testing.assert_array_equal(e.assignment(2)[0], idx)
        np.testing.assert_array_equal(e.assignment(2)[1], cost)


def test_solve_flat_returns_the_oracle_derived_winner(emu_lib, oracle_built):
    from oracle.dsa_oracle import OracleDsa
    from pydcop_amd import api
    name, make, kw, dsa_kw, infinity, every = R.best_cases()[1]
    g = make()
    seeds = list(range(5, 13))
    records, finals = R.oracle_records(OracleDsa, g, Params(**kw), dsa_kw, seeds, 24, every, infinity)
    w = R.winner(records, False)
    res = api.solve_flat(g, "min", 24, algo="dsa", seed=5, restarts=8, best_every=1, infinity=infinity, lib_path=emu_lib,
                         **dsa_kw)
    assert (res["replica"], res["best_cycle"]) == (w, records[w][2]) and res["best_cycle"] < 24
    assert [res["assignment"][n] for n in g.var_names] == [g.domains[i][x] for i, x in enumerate(records[w][3])]
    assert (res["violation"], res["cost"]) == records[w][:2]                  # mxs_dsa_eval_cost of that assignment
    assert res["replica_costs"] == [f[1] for f in finals]                       # the final states' costs
    # without tracking: the best final state
    res = api.solve_flat(g, "min", 24, algo="dsa", seed=5, restarts=8, infinity=infinity, lib_path=emu_lib, **dsa_kw)
    w = R.winner(finals, False)
    assert (res["replica"], res["best_cycle"]) == (w, 24) and (res["violation"], res["cost"]) == finals[w][:2]
    # the defaults: the single run, no new keys
    res = api.solve_flat(g, "min", 24, algo="dsa", seed=5, infinity=infinity, lib_path=emu_lib, **dsa_kw)
    assert "replica" not in res and (res["violation"], res["cost"]) == finals[0][:2]
    with pytest.raises(ValueError, match="dsa"):
        api.solve_flat(g, "min", 5, algo="mgm", restarts=2, lib_path=emu_lib)


# ---- behind pyDCOP

EDGES = [(1, 2), (2, 3), (3, 4), (4, 5), (5, 1), (2, 6), (6, 7), (3, 7), (8, 1), (8, 9), (9, 10), (10, 4), (7, 10), (5, 9)]


def soft_coloring_yaml(path):
    """Ten variables, three colours, a cost of 1 .. 5 on every edge whose ends agree."""
    lines = ["name: soft coloring", "objective: min", "domains:", "  colors:", "    values: [R, G, B]", "variables:"]
    for i in range(1, 11):
        lines += [f"  v{i:02d}:", "    domain: colors"]
    lines.append("constraints:")
    for k, (a, b) in enumerate(EDGES):
        lines += [f"  diff_{a:02d}_{b:02d}:", "    type: intention",
                  f"    function: {1 + k % 5} if v{a:02d} == v{b:02d} else 0"]
    lines.append("agents:")
    for i in range(1, 12):
        lines += [f"  a{i:02d}:", "    capacity: 100"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return str(path)


@pytest.fixture(scope="module")
def pydcop_ready(emu_lib):
    import sys
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from pydcop_amd import plugin
    plugin.install()
    from pydcop.algorithms import load_algorithm_module
    mod = load_algorithm_module("dsa_gpu")
    from pydcop_amd import engine
    before = engine.DEFAULT_LIB
    engine.register_test_engine(emu_lib, make_default=True)
    yield mod
    engine.DEFAULT_LIB = before


@needs_pydcop
def test_dsa_gpu_parameters(pydcop_ready):
    from pydcop.algorithms import load_algorithm_module
    ref = load_algorithm_module("dsa")
    refp = {p.name: (p.type, p.values, p.default_value) for p in ref.algo_params}
    mine = {p.name: (p.type, p.values, p.default_value) for p in pydcop_ready.algo_params}
    assert all(mine[k] == v for k, v in refp.items())
    assert set(mine) - set(refp) == {"precision", "seed", "chunk", "restarts", "best_every"}
    assert mine["restarts"] == ("int", None, 1) and mine["best_every"] == ("int", None, 0)


@needs_pydcop
@pytest.mark.parametrize("best_every", [0, 1])
def test_dsa_gpu_with_restarts_reports_the_best_replica(pydcop_ready, tmp_path, best_every):
    from pydcop.algorithms import AlgorithmDef
    from pydcop.dcop.yamldcop import load_dcop_from_file
    from pydcop.infrastructure.run import solve
    from pydcop_amd.algorithms.mgm2_gpu import compile_dcop_for_local_search
    from pydcop_amd.compile import assignment_to_values
    path = soft_coloring_yaml(tmp_path / "soft.yaml")
    dcop = load_dcop_from_file([path])
    algo = AlgorithmDef.build_with_default_param(
        "dsa_gpu", {"stop_cycle": 9, "variant": "C", "seed": 4, "restarts": 4, "best_every": best_every}, mode="min")
    got = solve(dcop, algo, "adhoc", timeout=20)
    g = compile_dcop_for_local_search(load_dcop_from_file([path]))
    with DsaEngine(g, Params(), variant="C", seed=4, replicas=4) as e:
        e.track_best(best_every, float("inf"))
        e.run(9)
        best = e.best()
        finals = [assignment_to_values(g, e.assignment(r)[0]) for r in range(4)]
        costs = e.replica_costs()[0]
    assert got == assignment_to_values(g, best["idx"])
    assert len({json.dumps(f, sort_keys=True) for f in finals}) > 1          # the replicas are different runs
    if best_every == 0:
        assert best["cost"] == costs.min() and got == finals[int(costs.argmin())]
    else:
        assert best["cost"] <= costs.min()


@needs_pydcop
def test_dsa_gpu_with_the_defaults_is_the_single_run(pydcop_ready, tmp_path):
    from pydcop.algorithms import AlgorithmDef
    from pydcop.dcop.yamldcop import load_dcop_from_file
    from pydcop.infrastructure.run import solve
    from pydcop_amd.algorithms.mgm2_gpu import compile_dcop_for_local_search
    from pydcop_amd.compile import assignment_to_values
    path = soft_coloring_yaml(tmp_path / "soft.yaml")
    algo = AlgorithmDef.build_with_default_param("dsa_gpu", {"stop_cycle": 9, "variant": "C", "seed": 4}, mode="min")
    got = solve(load_dcop_from_file([path]), algo, "adhoc", timeout=20)
    g = compile_dcop_for_local_search(load_dcop_from_file([path]))
    with DsaEngine(g, Params(), variant="C", seed=4) as e:
        e.run(9)
        assert got == assignment_to_values(g, e.assignment()[0])


@needs_pydcop
def test_cli_takes_restarts_and_best_every(pydcop_ready, tmp_path, capsys):
    """`python -m pydcop_amd.api -a dsa -p restarts:8 -p best_every:5` on a YAML DCOP: solve_dcop's result"""
    from pydcop.dcop.yamldcop import load_dcop_from_file
    from pydcop_amd import api
    path = soft_coloring_yaml(tmp_path / "soft.yaml")
    api.main(["-a", "dsa", "-c", "20", "-p", "restarts:8", "-p", "best_every:5", "-p", "seed:3", "-p", "variant:C", path])
    out = json.loads(capsys.readouterr().out)
    assert out["status"] == "FINISHED" and 0 <= out["replica"] < 8 and out["best_cycle"] in (0, 5, 10, 15, 20)
    assert len(out["replica_costs"]) == 8 and out["cost"] <= min(out["replica_costs"])
    res = api.solve_dcop(load_dcop_from_file([path]), 20, algo="dsa", seed=3, variant="C", restarts=8, best_every=5)
    assert res["assignment"] == out["assignment"] and res["cost"] == out["cost"]
    # DCOP.solution_cost of the returned assignment, not the device's number (here they agree: integers)
    assert res["violation"] == 0 and res["cost"] == float(res["cost"])
