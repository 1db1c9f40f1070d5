"""MGM's keyed draws and replicas above the engine, on the emulated build: the refusals of the C-ABI and of the binding,
`solve_flat` / the CLI with `draws` and `restarts`, and the `mgm_gpu` plug-in behind an unmodified pyDCOP against the
reference's own MgmComputation under the same keyed generator (those need the reference checkout)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

from dsa_replicas_common import winner
from mgm_keyed_oracle import OracleMgmKeyed
from oracle.stage_reference import locate as _locate_reference
from pydcop_amd import generators as G
from pydcop_amd.engine import MaxSumGpuError, load_library
from pydcop_amd.graph import Params
from pydcop_amd.mgm import MgmEngine

REF = _locate_reference() or ""
INST = os.path.join(REF, "tests", "instances")
needs_pydcop = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "pydcop")),
                                  reason="the pyDCOP reference checkout is not on this machine")
MXS_E_INVALID = -1


@pytest.fixture(scope="module")
def emu_lib():
    from emu.build_emu import build
    return build()


def test_c_abi_refusals(emu_lib):
    lib = load_library(emu_lib)
    assert lib.mxs_version() == 270
    g = G.random_coloring(12, seed=1)
    cg, cp = g.to_c(), Params().to_c()
    seeds = np.arange(4097, dtype=np.uint64)
    for n in (0, 4097, -3):
        h = C.c_void_p()
        rc = lib.mxs_mgm_create_keyed(C.byref(cg), C.byref(cp), None, seeds.ctypes.data, n, 0, C.byref(h))
        assert rc == MXS_E_INVALID and not h.value, n
        assert "replicas" in lib.mxs_last_error().decode()
    h = C.c_void_p()
    assert lib.mxs_mgm_create_keyed(C.byref(cg), C.byref(cp), None, None, 2, 0, C.byref(h)) == MXS_E_INVALID
    assert lib.mxs_mgm_create_keyed(C.byref(cg), C.byref(cp), None, seeds.ctypes.data, 3, 0, C.byref(h)) == 0
    n = C.c_int32(0)
    assert lib.mxs_mgm_replicas(h, C.byref(n)) == 0 and n.value == 3
    idx = np.empty(g.n_vars, dtype=np.int32)
    for r in (-1, 3):
        assert lib.mxs_mgm_get_state_replica(h, r, idx.ctypes.data, None, None, None, None) == MXS_E_INVALID
    assert lib.mxs_mgm_get_state_replica(h, 2, idx.ctypes.data, None, None, None, None) == 0
    assert lib.mxs_mgm_destroy(h) == 0
    # an engine of mxs_mgm_create has one replica
    assert lib.mxs_mgm_create(C.byref(cg), C.byref(cp), None, 0, C.byref(h)) == 0
    assert lib.mxs_mgm_replicas(h, C.byref(n)) == 0 and n.value == 1
    assert lib.mxs_mgm_get_state_replica(h, 1, idx.ctypes.data, None, None, None, None) == MXS_E_INVALID
    assert lib.mxs_mgm_destroy(h) == 0


def test_binding_refusals(emu_lib):
    g = G.random_coloring(12, seed=1)
    with pytest.raises(ValueError, match="keyed"):
        MgmEngine(g, replicas=3, draws="fixed", lib_path=emu_lib)
    with pytest.raises(ValueError, match="keyed"):
        MgmEngine(g, seeds=[4], lib_path=emu_lib)
    with pytest.raises(ValueError, match="seeds"):
        MgmEngine(g, draws="keyed", replicas=3, seeds=[1, 2], lib_path=emu_lib)
    with pytest.raises(ValueError, match="draws"):
        MgmEngine(g, draws="random", lib_path=emu_lib)
    with pytest.raises(MaxSumGpuError, match="replicas"):
        MgmEngine(g, draws="keyed", replicas=0, lib_path=emu_lib)
    with MgmEngine(g, draws="keyed", replicas=2, lib_path=emu_lib) as e:
        with pytest.raises(MaxSumGpuError, match="replica"):
            e.state(2)


def test_a_library_without_the_keyed_entry_points_says_so(emu_lib, monkeypatch):
    """a library built from older sources loads (the fixed draws work) and is refused by name for draws="keyed\""""
    import pydcop_amd.mgm as M

    class Old:
        def __init__(self, lib):
            self._lib, self._name = lib, "libmaxsum_hip_old.so"

        def __getattr__(self, name):
            if name in M.KEYED_SYMBOLS:
                raise AttributeError(name)
            return getattr(self._lib, name)

    monkeypatch.setattr(M, "load_library", lambda path=None: Old(load_library(emu_lib)))
    g = G.random_coloring(12, seed=1)
    with MgmEngine(g) as e:
        e.run(2)
    with pytest.raises(MaxSumGpuError, match="mxs_mgm_create_keyed"):
        MgmEngine(g, draws="keyed")


def oracle_finals(g, params, seeds, rounds, infinity):
    out = []
    for s in seeds:
        o = OracleMgmKeyed(g, params, draws="keyed", seed=s)
        o.run(rounds)
        idx = o.state()["idx"]
        cost, viol = o.eval_cost(idx, infinity)
        out.append((viol, cost, idx))
    return out


def test_solve_flat_returns_the_oracle_derived_winner(emu_lib, oracle_built):
    from oracle.mgm_oracle import OracleMgm
    from pydcop_amd import api
    g = G.random_coloring(60, seed=32, variant="hard", unary_noise=0)
    finals = oracle_finals(g, Params(), range(5, 13), 12, 1000.0)
    w = winner(finals, False)
    assert len({f[:2] for f in finals}) > 1
    res = api.solve_flat(g, "min", 12, algo="mgm", draws="keyed", seed=5, restarts=8, infinity=1000.0, lib_path=emu_lib)
    assert res["replica"] == w and "best_cycle" not in res
    assert [res["assignment"][n] for n in g.var_names] == [g.domains[i][x] for i, x in enumerate(finals[w][2])]
    assert (res["violation"], res["cost"]) == finals[w][:2]
    assert res["replica_costs"] == [f[1] for f in finals]
    # keyed, one run: that run, no new keys
    res = api.solve_flat(g, "min", 12, algo="mgm", draws="keyed", seed=7, infinity=1000.0, lib_path=emu_lib)
    assert "replica" not in res and (res["violation"], res["cost"]) == finals[2][:2]
    # the defaults: the fixed-draw run, no new keys
    o = OracleMgm(g, Params())
    o.run(12)
    cost, viol = o.eval_cost(infinity=1000.0)
    res = api.solve_flat(g, "min", 12, algo="mgm", infinity=1000.0, lib_path=emu_lib)
    assert "replica" not in res and "replica_costs" not in res and (res["violation"], res["cost"]) == (viol, cost)
    assert [res["assignment"][n] for n in g.var_names] == [g.domains[i][x] for i, x in enumerate(o.state()["idx"])]
    o.close()
    with pytest.raises(ValueError, match="dsa"):
        api.solve_flat(g, "min", 5, algo="mgm", restarts=2, lib_path=emu_lib)
    with pytest.raises(ValueError, match="best_every"):
        api.solve_flat(g, "min", 5, algo="mgm", draws="keyed", restarts=2, best_every=1, lib_path=emu_lib)
    with pytest.raises(ValueError, match="draws"):
        api.solve_flat(g, "min", 5, algo="dsa", draws="keyed", lib_path=emu_lib)


def test_cli_round_trip_on_an_instance_file(emu_lib, tmp_path, capsys):
    """`python -m pydcop_amd.api -a mgm -p draws:keyed -p seed:3 -p restarts:8 instance.npz`: solve_flat's result, and
    the seed reaches the engine (the .npz path used to drop it for MGM)"""
    from pydcop_amd import api, engine
    g = G.random_coloring(60, seed=32, variant="hard", unary_noise=0)
    path = str(tmp_path / "hard.npz")
    g.save(path, objective="min")
    before = engine.DEFAULT_LIB
    engine.register_test_engine(emu_lib, make_default=True)
    try:
        outs = {}
        for seed in (3, 4):
            api.main(["-a", "mgm", "-c", "12", "--infinity", "1000", "-p", "draws:keyed", "-p", f"seed:{seed}", "-p",
                      "restarts:8", path])
            outs[seed] = json.loads(capsys.readouterr().out)
        res = api.solve_flat(g, "min", 12, algo="mgm", draws="keyed", seed=3, restarts=8, infinity=1000.0)
    finally:
        engine.DEFAULT_LIB = before
    out = outs[3]
    assert out["status"] == "FINISHED" and out["assignment"] == res["assignment"]
    assert (out["replica"], out["replica_costs"], out["cost"], out["violation"]) == (
        res["replica"], res["replica_costs"], res["cost"], res["violation"])
    finals = oracle_finals(g, Params(), range(3, 11), 12, 1000.0)
    assert out["replica_costs"] == [f[1] for f in finals] and out["replica"] == winner(finals, False)
    assert outs[4]["replica_costs"] == out["replica_costs"][1:] + [oracle_finals(g, Params(), [11], 12, 1000.0)[0][1]]


# ---- behind pyDCOP

@pytest.fixture(scope="module")
def pydcop_ready(emu_lib):
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from pydcop_amd import plugin
    plugin.install()
    from pydcop.algorithms import load_algorithm_module
    mod = load_algorithm_module("mgm_gpu")
    from pydcop_amd import engine
    before = engine.DEFAULT_LIB
    engine.register_test_engine(emu_lib, make_default=True)
    yield mod
    engine.DEFAULT_LIB = before


@needs_pydcop
def test_mgm_gpu_parameters(pydcop_ready):
    from pydcop.algorithms import load_algorithm_module
    ref = load_algorithm_module("mgm")
    refp = {p.name: (p.type, p.values, p.default_value) for p in ref.algo_params}
    mine = {p.name: (p.type, p.values, p.default_value) for p in pydcop_ready.algo_params}
    assert all(mine[k] == v for k, v in refp.items())
    assert set(mine) - set(refp) == {"precision", "chunk", "draws", "seed", "restarts"}
    assert mine["draws"] == ("str", ["fixed", "keyed"], "fixed")
    assert mine["seed"] == ("int", None, 0) and mine["restarts"] == ("int", None, 1)


@needs_pydcop
@pytest.mark.parametrize("instance", ["graph_coloring_tuto.yaml", "graph_coloring_3agts_10vars.yaml"])
def test_mgm_gpu_with_keyed_draws_equals_the_reference(pydcop_ready, instance):
    """`--algo mgm_gpu` with draws:keyed through the unmodified orchestrator / agents == the reference's own
    MgmComputation objects drawing from the same keyed generator (the variables indexed by sorted name), after the
    same number of rounds"""
    from mgm_keyed_reference import run_reference_mgm_keyed
    from pydcop.algorithms import AlgorithmDef
    from pydcop.dcop.yamldcop import load_dcop_from_file
    from pydcop.infrastructure.run import solve
    dcop = load_dcop_from_file([os.path.join(INST, instance)])
    algo = AlgorithmDef.build_with_default_param("mgm_gpu", {"draws": "keyed", "seed": 3, "stop_cycle": 9},
                                                 mode=dcop.objective)
    got = solve(dcop, algo, "adhoc", timeout=5)
    want, _, _, _ = run_reference_mgm_keyed(load_dcop_from_file([os.path.join(INST, instance)]), 8, seed=3)
    assert got == want


@needs_pydcop
def test_mgm_gpu_with_restarts_publishes_the_best_replica(pydcop_ready):
    from pydcop.algorithms import AlgorithmDef
    from pydcop.dcop.yamldcop import load_dcop_from_file
    from pydcop.infrastructure.run import solve
    from pydcop_amd.algorithms.mgm2_gpu import compile_dcop_for_local_search
    from pydcop_amd.compile import assignment_to_values
    path = os.path.join(INST, "graph_coloring_3agts_10vars.yaml")
    dcop = load_dcop_from_file([path])
    algo = AlgorithmDef.build_with_default_param("mgm_gpu", {"draws": "keyed", "seed": 4, "restarts": 6, "stop_cycle": 9},
                                                 mode=dcop.objective)
    got = solve(dcop, algo, "adhoc", timeout=5)
    g = compile_dcop_for_local_search(load_dcop_from_file([path]))
    with MgmEngine(g, Params(mode=dcop.objective), draws="keyed", seed=4, replicas=6) as e:
        e.run(8)
        best = e.best()
        costs = e.replica_costs()[0]
    assert got == assignment_to_values(g, best["idx"])
    assert best["cost"] == (costs.max() if dcop.objective == "max" else costs.min())
    with pytest.raises(ValueError, match="draws"):               # the parameter table refuses other values
        AlgorithmDef.build_with_default_param("mgm_gpu", {"draws": "sometimes"}, mode=dcop.objective)
