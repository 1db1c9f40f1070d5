"""`--algo gdba_gpu` behind an UNMODIFIED pyDCOP, on the emulated engine (no GPU here): the reference's
orchestrator and agents drive the plug-in, and the result equals the reference's own GdbaComputation
objects under the same keyed draws (tests/gdba_reference.py) -- as tests/test_mgm2_plugin.py does for
MGM-2.  Needs the reference checkout."""
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
    mod = load_algorithm_module("gdba_gpu")
    from pydcop_amd import engine
    before = engine.DEFAULT_LIB
    engine.register_test_engine(emu_lib, make_default=True)
    yield mod
    engine.DEFAULT_LIB = before


def test_pydcop_lists_gdba_gpu(pydcop_ready):
    from pydcop.algorithms import list_available_algorithms
    assert "gdba_gpu" in list_available_algorithms() and "gdba" in list_available_algorithms()


def test_module_attributes_like_the_reference(pydcop_ready):
    from pydcop.algorithms import load_algorithm_module
    ref, mod = load_algorithm_module("gdba"), pydcop_ready
    assert mod.GRAPH_TYPE == ref.GRAPH_TYPE == "constraints_hypergraph"
    assert (mod.UNIT_SIZE, mod.HEADER_SIZE) == (ref.UNIT_SIZE, ref.HEADER_SIZE)
    refp = {p.name: (p.type, p.values, p.default_value) for p in ref.algo_params}
    mine = {p.name: (p.type, p.values, p.default_value) for p in mod.algo_params}
    assert len(refp) == 3 and all(mine[k] == v for k, v in refp.items())
    assert set(mine) - set(refp) == {"stop_cycle", "precision", "seed", "chunk"}


def test_parameters_validate_and_default_like_gdba(pydcop_ready):
    from pydcop.algorithms import AlgorithmDef
    ref = AlgorithmDef.build_with_default_param("gdba", {"violation": "MX"}, mode="min")
    mine = AlgorithmDef.build_with_default_param("gdba_gpu", {"violation": "MX"}, mode="min")
    for k in ("modifier", "violation", "increase_mode"):
        assert mine.params[k] == ref.params[k]
    assert (mine.params["stop_cycle"], mine.params["precision"], mine.params["seed"]) == (0, "f64", 0)
    for bad in ({"modifier": "X"}, {"violation": "ZZ"}, {"increase_mode": "Q"}, {"precision": "f16"}):
        with pytest.raises(ValueError):
            AlgorithmDef.build_with_default_param("gdba_gpu", bad, mode="min")
        if "precision" not in bad:
            with pytest.raises(ValueError):
                AlgorithmDef.build_with_default_param("gdba", bad, mode="min")


@pytest.mark.parametrize("instance,kw", [
    ("graph_coloring1.yaml", dict(modifier="A", violation="NZ", increase_mode="E")),
    ("graph_coloring_tuto.yaml", dict(modifier="M", violation="NM", increase_mode="T")),
    ("graph_coloring_3agts_10vars.yaml", dict(modifier="A", violation="MX", increase_mode="R")),
    ("graph_coloring_tuto_max.yaml", dict(modifier="M", violation="NZ", increase_mode="C"))])
def test_gdba_gpu_equals_the_reference_gdba(pydcop_ready, instance, kw):
    from gdba_reference import run_reference_gdba
    from pydcop.algorithms import AlgorithmDef
    from pydcop.dcop.yamldcop import load_dcop_from_file
    from pydcop.infrastructure.run import solve
    dcop = load_dcop_from_file([os.path.join(INST, instance)])
    algo = AlgorithmDef.build_with_default_param("gdba_gpu", dict(kw, stop_cycle=9, seed=3), mode=dcop.objective)
    got = solve(dcop, algo, "adhoc", timeout=5)
    dcop2 = load_dcop_from_file([os.path.join(INST, instance)])
    want, _, _, _ = run_reference_gdba(dcop2, 8, seed=3, **kw)
    assert got == want


def test_footprint_and_load_like_the_reference(pydcop_ready):
    from pydcop.algorithms import load_algorithm_module
    from pydcop.computations_graph import constraints_hypergraph as chg
    from pydcop.dcop.yamldcop import load_dcop_from_file
    ref, mod = load_algorithm_module("gdba"), pydcop_ready
    mgm = load_algorithm_module("mgm")
    cg = chg.build_computation_graph(load_dcop_from_file([os.path.join(INST, "graph_coloring_tuto.yaml")]))
    for node in cg.nodes:
        # gdba.computation_memory itself raises on a real node (it takes neighbour names for links); its formula,
        # one UNIT_SIZE per neighbour, is the one mgm.py computes over the links
        with pytest.raises(AttributeError):
            ref.computation_memory(node)
        assert mod.computation_memory(node) == mgm.computation_memory(node) == len(node.neighbors) * ref.UNIT_SIZE
        for other in node.neighbors:
            assert mod.communication_load(node, other) == ref.communication_load(node, other)


def test_api_runs_gdba(pydcop_ready, capsys):
    """`python -m pydcop_amd.api -a gdba -p modifier:... -p violation:... -p increase_mode:...` on a YAML DCOP."""
    from pydcop_amd import api
    api.main(["-a", "gdba", "-c", "6", "-p", "modifier:M", "-p", "violation:NM", "-p", "increase_mode:T", "-p", "seed:2",
              os.path.join(INST, "graph_coloring_tuto.yaml")])
    out = json.loads(capsys.readouterr().out)
    assert out["status"] == "FINISHED" and out["cycle"] == 6
    assert set(out["assignment"]) == {"v1", "v2", "v3", "v4"}
