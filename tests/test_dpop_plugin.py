"""dpop_gpu through the UNMODIFIED orchestrator (pydcop.infrastructure.run.solve, thread agents) on the
emulated engine: the assignment of the reference's own `dpop` on the reference's instances; the module's
contract attributes; `python -m pydcop_amd.api -a dpop`.  Skipped without the reference checkout."""
import json
import os

import pytest

from oracle import ref_harness

pytestmark = pytest.mark.skipif(not ref_harness.reference_available(), reason="reference tree not present")


@pytest.fixture(scope="module", autouse=True)
def pydcop_ready():
    """the reference importable, the plug-in installed, the emulated engine the default library"""
    from emu.build_emu import build
    emu_lib = build()
    ref_harness.install_shims()      # (the reference's own dpop needs ndarray.itemset, gone in numpy 2)
    from pydcop_amd import engine, plugin
    plugin.install()
    before = engine.DEFAULT_LIB
    engine.register_test_engine(emu_lib, make_default=True)
    yield
    engine.DEFAULT_LIB = before

INSTANCES = ["graph_coloring1.yaml", "graph_coloring_tuto.yaml", "graph_coloring_tuto_max.yaml",
             "graph_coloring_3agts_10vars.yaml", "secp_simple1.yaml"]


def _load(instance):
    from pydcop_amd import plugin
    plugin.install()
    from pydcop.dcop.objects import AgentDef
    from pydcop.dcop.yamldcop import load_dcop_from_file
    dcop = load_dcop_from_file([os.path.join(ref_harness.REFERENCE_ROOT, "tests", "instances", instance)])
    # DPOP defines no footprint, so only `oneagent` distributes it: one agent per computation, which
    # graph_coloring_3agts_10vars lacks -- the problem is unchanged by the extra hosts
    for i in range(len(dcop.variables) - len(dcop.agents)):
        dcop.add_agents([AgentDef(f"extra_agent_{i}")])
    return dcop


@pytest.mark.parametrize("instance", INSTANCES)
def test_dpop_gpu_equals_reference_dpop_through_the_orchestrator(instance):
    from pydcop.infrastructure.run import solve
    got = solve(_load(instance), "dpop_gpu", "oneagent", timeout=4)
    want = solve(_load(instance), "dpop", "oneagent", timeout=4)
    assert got == want


@pytest.mark.parametrize("instance", INSTANCES)
def test_api_dpop_equals_reference_dpop(instance, capsys):
    from pydcop.infrastructure.run import solve
    from pydcop_amd import api
    want = solve(_load(instance), "dpop", "oneagent", timeout=4)
    path = os.path.join(ref_harness.REFERENCE_ROOT, "tests", "instances", instance)
    capsys.readouterr()
    api.main(["-a", "dpop", "-c", "7", path])
    out = json.loads(capsys.readouterr().out)
    assert out["assignment"] == want and out["cycle"] == 0 and out["status"] == "FINISHED"
    res = api.solve_dcop_dpop(_load(instance), precision="f32")
    assert res["assignment"] == want


def test_dpop_gpu_module_contract():
    from pydcop_amd import plugin
    plugin.install()
    from pydcop.algorithms import list_available_algorithms, load_algorithm_module
    assert "dpop_gpu" in list_available_algorithms()
    m = load_algorithm_module("dpop_gpu")
    assert m.GRAPH_TYPE == "pseudotree"
    assert sorted(p.name for p in m.algo_params) == ["max_bytes", "precision"]
    with pytest.raises(NotImplementedError):
        m.computation_memory(None)
    with pytest.raises(NotImplementedError):
        m.communication_load(None, "x")
    from pydcop_amd.algorithms import maxsum_gpu
    assert "dpop_gpu" in maxsum_gpu.SESSION_CLASSES


def test_dpop_gpu_refuses_over_budget_through_the_session():
    """`max_bytes` reaches the engine: a budget of one byte refuses any instance with a UTIL"""
    from pydcop.algorithms import AlgorithmDef, ComputationDef, load_algorithm_module
    from pydcop.computations_graph import pseudotree
    from pydcop_amd.engine import MaxSumGpuError
    dcop = _load("graph_coloring1.yaml")
    m = load_algorithm_module("dpop_gpu")
    algo = AlgorithmDef.build_with_default_param("dpop_gpu", {"max_bytes": 1}, mode=dcop.objective)
    comps = [m.build_computation(ComputationDef(n, algo)) for n in pseudotree.build_computation_graph(dcop).nodes]
    with pytest.raises(MaxSumGpuError, match="over the budget of 1 bytes"):
        comps[0]._session._open()
