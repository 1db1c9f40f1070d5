"""MGM-2's replicas above the engine, on the emulated build: `solve_flat` / the CLI with `restarts`, a library without
the new entry points, and the `mgm2_gpu` plug-in with `restarts` behind an unmodified pyDCOP (that needs the reference
checkout)."""
import json
import os
import sys

import pytest

from dsa_replicas_common import winner
from mgm2_replicas_common import oracle_finals
from oracle.stage_reference import locate as _locate_reference
from pydcop_amd import generators as G
from pydcop_amd.engine import MaxSumGpuError, load_library
from pydcop_amd.graph import Params
from pydcop_amd.mgm2 import Mgm2Engine

REF = _locate_reference() or ""
INST = os.path.join(REF, "tests", "instances")
needs_pydcop = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "pydcop")),
                                  reason="the pyDCOP reference checkout is not on this machine")


@pytest.fixture(scope="module")
def emu_lib():
    from emu.build_emu import build
    return build()


def hard():
    return G.random_coloring(45, seed=31, variant="hard", unary_noise=0)


def test_solve_flat_returns_the_oracle_derived_winner(emu_lib):
    from pydcop_amd import api
    g, kw = hard(), dict(favor="coordinated")
    finals = oracle_finals(g, Params(), kw, range(5, 13), 12, 1000.0)
    w = winner(finals, False)
    assert len({f[:2] for f in finals}) > 1
    res = api.solve_flat(g, "min", 12, algo="mgm2", seed=5, restarts=8, infinity=1000.0, lib_path=emu_lib, **kw)
    assert res["replica"] == w and "best_cycle" not in res
    assert [res["assignment"][n] for n in g.var_names] == [g.domains[i][x] for i, x in enumerate(finals[w][2])]
    assert (res["violation"], res["cost"]) == finals[w][:2]
    assert res["replica_costs"] == [f[1] for f in finals]
    # one run: that run, through mxs_mgm2_create as before, no new keys
    res = api.solve_flat(g, "min", 12, algo="mgm2", seed=7, restarts=1, infinity=1000.0, lib_path=emu_lib, **kw)
    assert "replica" not in res and "replica_costs" not in res
    assert (res["violation"], res["cost"]) == finals[2][:2]
    assert [res["assignment"][n] for n in g.var_names] == [g.domains[i][x] for i, x in enumerate(finals[2][2])]
    assert res == api.solve_flat(g, "min", 12, algo="mgm2", seed=7, infinity=1000.0, lib_path=emu_lib, **kw)
    # what stays refused, in the words the other engines' tests look for
    with pytest.raises(ValueError, match="dsa"):
        api.solve_flat(g, "min", 5, algo="mgm", restarts=2, lib_path=emu_lib)
    with pytest.raises(ValueError, match="dsa"):
        api.solve_flat(g, "min", 5, algo="gdba", restarts=2, lib_path=emu_lib)
    with pytest.raises(ValueError, match="best_every"):
        api.solve_flat(g, "min", 5, algo="mgm2", restarts=2, best_every=1, lib_path=emu_lib)
    with pytest.raises(ValueError, match="draws"):
        api.solve_flat(g, "min", 5, algo="mgm2", draws="keyed", lib_path=emu_lib)


def test_cli_round_trip_on_an_instance_file(emu_lib, tmp_path, capsys):
    """`python -m pydcop_amd.api -a mgm2 -p seed:3 -p restarts:8 instance.npz`: solve_flat's result"""
    from pydcop_amd import api, engine
    g = hard()
    path = str(tmp_path / "hard.npz")
    g.save(path, objective="min")
    before = engine.DEFAULT_LIB
    engine.register_test_engine(emu_lib, make_default=True)
    try:
        api.main(["-a", "mgm2", "-c", "12", "--infinity", "1000", "-p", "favor:coordinated", "-p", "seed:3", "-p",
                  "restarts:8", path])
        out = json.loads(capsys.readouterr().out)
        res = api.solve_flat(g, "min", 12, algo="mgm2", favor="coordinated", seed=3, restarts=8, infinity=1000.0)
    finally:
        engine.DEFAULT_LIB = before
    assert out["status"] == "FINISHED" and out["assignment"] == res["assignment"]
    assert (out["replica"], out["replica_costs"], out["cost"], out["violation"]) == (
        res["replica"], res["replica_costs"], res["cost"], res["violation"])
    finals = oracle_finals(g, Params(), dict(favor="coordinated"), range(3, 11), 12, 1000.0)
    assert out["replica_costs"] == [f[1] for f in finals] and out["replica"] == winner(finals, False)
    assert (out["violation"], out["cost"]) == finals[out["replica"]][:2]


def test_a_library_without_the_replica_entry_points_says_so(emu_lib, monkeypatch):
    """a library built from older sources loads (the single run works) and is refused by name for replicas"""
    import pydcop_amd.mgm2 as M

    class Old:
        def __init__(self, lib):
            self._lib, self._name = lib, "libmaxsum_hip_old.so"

        def __getattr__(self, name):
            if name in M.REPLICA_SYMBOLS:
                raise AttributeError(name)
            return getattr(self._lib, name)

    monkeypatch.setattr(M, "load_library", lambda path=None: Old(load_library(emu_lib)))
    g = G.random_coloring(12, seed=1)
    with Mgm2Engine(g) as e:
        e.run(2)
        with pytest.raises(MaxSumGpuError, match="mxs_mgm2_replica_costs"):
            e.replica_costs()
    with pytest.raises(MaxSumGpuError, match="mxs_mgm2_create_replicas"):
        Mgm2Engine(g, replicas=2)


# ---- behind pyDCOP

@pytest.fixture(scope="module")
def pydcop_ready(emu_lib):
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from pydcop_amd import plugin
    plugin.install()
    from pydcop.algorithms import load_algorithm_module
    mod = load_algorithm_module("mgm2_gpu")
    from pydcop_amd import engine
    before = engine.DEFAULT_LIB
    engine.register_test_engine(emu_lib, make_default=True)
    yield mod
    engine.DEFAULT_LIB = before


@needs_pydcop
def test_mgm2_gpu_parameters(pydcop_ready):
    from pydcop.algorithms import load_algorithm_module
    ref = load_algorithm_module("mgm2")
    refp = {p.name: (p.type, p.values, p.default_value) for p in ref.algo_params}
    mine = {p.name: (p.type, p.values, p.default_value) for p in pydcop_ready.algo_params}
    assert all(mine[k] == v for k, v in refp.items())
    assert set(mine) - set(refp) == {"precision", "seed", "chunk", "restarts"}
    assert mine["restarts"] == ("int", None, 1)


@needs_pydcop
def test_mgm2_gpu_with_restarts_publishes_the_best_replica(pydcop_ready):
    from pydcop.algorithms import AlgorithmDef
    from pydcop.dcop.yamldcop import load_dcop_from_file
    from pydcop.infrastructure.run import solve
    from pydcop_amd.algorithms.mgm2_gpu import compile_dcop_for_local_search
    from pydcop_amd.compile import assignment_to_values
    path = os.path.join(INST, "graph_coloring_3agts_10vars.yaml")
    dcop = load_dcop_from_file([path])
    algo = AlgorithmDef.build_with_default_param("mgm2_gpu", {"favor": "coordinated", "seed": 4, "restarts": 4,
                                                              "stop_cycle": 9}, mode=dcop.objective)
    got = solve(dcop, algo, "adhoc", timeout=5)
    g = compile_dcop_for_local_search(load_dcop_from_file([path]))
    with Mgm2Engine(g, Params(mode=dcop.objective), favor="coordinated", seed=4, replicas=4) as e:
        e.run(8)
        best = e.best()
        costs = e.replica_costs()[0]
    assert got == assignment_to_values(g, best["idx"])
    assert best["cost"] == (costs.max() if dcop.objective == "max" else costs.min())
