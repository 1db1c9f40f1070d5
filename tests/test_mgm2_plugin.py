"""`--algo mgm2_gpu` behind an UNMODIFIED pyDCOP, on the emulated engine (no GPU here): the reference's
orchestrator and agents drive the plug-in, and the result equals the reference's own Mgm2Computation
objects under the same keyed draws (tests/mgm2_reference.py) -- as tests/test_plugin.py does for MGM.
Needs the reference checkout."""
import json
import os

import pytest

from oracle.stage_reference import locate as _locate_reference

REF = _locate_reference() or "/root/reference"
INST = os.path.join(REF, "tests", "instances")

pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "pydcop")),
                                reason="the pyDCOP reference checkout is not on this machine")


@pytest.fixture(scope="module")
def pydcop_ready():
    import sys
    from emu.build_emu import build
    emu_lib = build()
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


def test_module_attributes_like_the_reference(pydcop_ready):
    from pydcop.algorithms import load_algorithm_module
    ref, mod = load_algorithm_module("mgm2"), pydcop_ready
    assert mod.GRAPH_TYPE == ref.GRAPH_TYPE == "constraints_hypergraph"
    assert (mod.UNIT_SIZE, mod.HEADER_SIZE) == (ref.UNIT_SIZE, ref.HEADER_SIZE)
    refp = {p.name: (p.type, p.values, p.default_value) for p in ref.algo_params}
    mine = {p.name: (p.type, p.values, p.default_value) for p in mod.algo_params}
    assert all(mine[k] == v for k, v in refp.items())


@pytest.mark.parametrize("instance,favor", [("graph_coloring1.yaml", "unilateral"), ("graph_coloring_tuto.yaml", "no"),
                                            ("graph_coloring_3agts_10vars.yaml", "coordinated"),
                                            ("graph_coloring_tuto_max.yaml", "unilateral")])
def test_mgm2_gpu_equals_the_reference_mgm2(pydcop_ready, instance, favor):
    from mgm2_reference import run_reference_mgm2
    from pydcop.algorithms import AlgorithmDef
    from pydcop.dcop.yamldcop import load_dcop_from_file
    from pydcop.infrastructure.run import solve
    dcop = load_dcop_from_file([os.path.join(INST, instance)])
    algo = AlgorithmDef.build_with_default_param("mgm2_gpu", {"stop_cycle": 9, "favor": favor, "seed": 3},
                                                 mode=dcop.objective)
    got = solve(dcop, algo, "adhoc", timeout=5)
    dcop2 = load_dcop_from_file([os.path.join(INST, instance)])
    want, _, _ = run_reference_mgm2(dcop2, 8, favor=favor, seed=3)
    assert got == want


def test_footprint_and_load_like_the_reference(pydcop_ready):
    from pydcop.algorithms import load_algorithm_module
    from pydcop.computations_graph import constraints_hypergraph as chg
    from pydcop.dcop.yamldcop import load_dcop_from_file
    ref, mod = load_algorithm_module("mgm2"), pydcop_ready
    cg = chg.build_computation_graph(load_dcop_from_file([os.path.join(INST, "graph_coloring_tuto.yaml")]))
    for node in cg.nodes:
        assert mod.computation_memory(node) == ref.computation_memory(node)
        for other in node.neighbors:
            assert mod.communication_load(node, other) == ref.communication_load(node, other)


def test_bad_parameters_are_refused(pydcop_ready):
    from pydcop.algorithms import AlgorithmDef
    with pytest.raises(ValueError):
        AlgorithmDef.build_with_default_param("mgm2_gpu", {"favor": "both"}, mode="min")
    from pydcop_amd import generators as G
    from pydcop_amd.graph import Params
    from pydcop_amd.mgm2 import Mgm2Engine
    with pytest.raises(ValueError, match="threshold"):
        Mgm2Engine(G.random_coloring(10, seed=0), Params(), threshold=-0.1)
    with pytest.raises(ValueError, match="threshold"):
        Mgm2Engine(G.random_coloring(10, seed=0), Params(), threshold="high")


def test_api_runs_mgm2(pydcop_ready, capsys):
    """`python -m pydcop_amd.api -a mgm2 -p threshold:... -p favor:...` on a YAML DCOP."""
    from pydcop_amd import api
    api.main(["-a", "mgm2", "-c", "6", "-p", "threshold:0.7", "-p", "favor:coordinated", "-p", "seed:2",
              os.path.join(INST, "graph_coloring_tuto.yaml")])
    out = json.loads(capsys.readouterr().out)
    assert out["status"] == "FINISHED" and out["cycle"] == 6
    assert set(out["assignment"]) == {"v1", "v2", "v3", "v4"}
