"""`--algo dba_gpu` behind an UNMODIFIED pyDCOP, on the emulated engine (no GPU here): the reference's
orchestrator and agents drive the plug-in, the run ends FINISHED once the engine has stopped, and the
result equals the engine's and the reference's own DbaComputation objects under the same keyed draws
(tests/dba_reference.py) -- as tests/test_gdba_plugin.py does for GDBA.  Needs the reference checkout."""
import json
import os

import pytest

import dba_common
from oracle.stage_reference import locate as _locate_reference

REF = _locate_reference() or ""

pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "pydcop")),
                                reason="the pyDCOP reference checkout is not on this machine")

EDGES = [(1, 2), (2, 3), (3, 4), (4, 5), (5, 1), (2, 6), (6, 7), (3, 7), (8, 1)]


def hard_coloring_yaml(path, objective="min"):
    """Eight variables, three colours, a cost of 1000 on every edge whose ends agree."""
    lines = ["name: hard coloring", f"objective: {objective}", "domains:", "  colors:", "    values: [R, G, B]", "variables:"]
    for i in range(1, 9):
        lines += [f"  v{i}:", "    domain: colors"]
    lines.append("constraints:")
    for a, b in EDGES:
        lines += [f"  diff_{a}_{b}:", "    type: intention", f"    function: 1000 if v{a} == v{b} else 0"]
    lines.append("agents:")
    for i in range(1, 10):
        lines += [f"  a{i}:", "    capacity: 100"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return str(path)


@pytest.fixture(scope="module")
def pydcop_ready():
    import sys
    emu_lib = dba_common.emu_lib()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from pydcop_amd import plugin
    plugin.install()
    from pydcop.algorithms import load_algorithm_module
    mod = load_algorithm_module("dba_gpu")
    from pydcop_amd import engine
    before = engine.DEFAULT_LIB
    engine.register_test_engine(emu_lib, make_default=True)
    yield mod
    engine.DEFAULT_LIB = before


def test_pydcop_lists_dba_gpu(pydcop_ready):
    from pydcop.algorithms import list_available_algorithms
    assert "dba_gpu" in list_available_algorithms() and "dba" in list_available_algorithms()


def test_module_attributes_like_the_reference(pydcop_ready):
    from pydcop.algorithms import load_algorithm_module
    ref, mod = load_algorithm_module("dba"), pydcop_ready
    assert mod.GRAPH_TYPE == ref.GRAPH_TYPE == "constraints_hypergraph"
    assert (mod.UNIT_SIZE, mod.HEADER_SIZE) == (ref.UNIT_SIZE, ref.HEADER_SIZE)
    refp = {p.name: (p.type, p.values, p.default_value) for p in ref.algo_params}
    mine = {p.name: (p.type, p.values, p.default_value) for p in mod.algo_params}
    assert len(refp) == 2 and all(mine[k] == v for k, v in refp.items())
    assert set(mine) - set(refp) == {"stop_cycle", "seed", "chunk"}


def test_dba_gpu_finishes_and_equals_the_engine_and_the_reference(pydcop_ready, tmp_path):
    from dba_reference import run_reference_dba
    from pydcop.algorithms import AlgorithmDef
    from pydcop.dcop.yamldcop import load_dcop_from_file
    from pydcop.infrastructure.run import solve
    from pydcop_amd.algorithms.mgm2_gpu import compile_dcop_for_local_search
    from pydcop_amd.compile import assignment_to_values
    from pydcop_amd.dba import DbaEngine
    from pydcop_amd.graph import Params
    path = hard_coloring_yaml(tmp_path / "hard.yaml")
    kw = dict(infinity=1000, max_distance=3)
    dcop = load_dcop_from_file([path])
    algo = AlgorithmDef.build_with_default_param("dba_gpu", dict(kw, seed=3, chunk=2), mode=dcop.objective)
    # no stop_cycle: `pydcop solve` ends by itself, FINISHED, once a termination counter has reached max_distance
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from pydcop_amd import plugin, engine; plugin.install()\n"
        "engine.register_test_engine(%r, make_default=True)\n"
        "sys.argv = ['pydcop', '-t', '30', 'solve', '--algo', 'dba_gpu', '-p', 'infinity:1000',\n"
        "            '-p', 'max_distance:3', '-p', 'seed:3', '-p', 'chunk:2', '-d', 'adhoc', %r]\n"
        "from pydcop import dcop_cli; dcop_cli.main()\n"
    ) % (root, REF, dba_common.emu_lib(), path)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout[out.stdout.index("{"):])
    assert res["status"] == "FINISHED" and res["violation"] == 0
    got = res["assignment"]
    g = compile_dcop_for_local_search(load_dcop_from_file([path]))
    with DbaEngine(g, Params(), seed=3, **kw) as e:
        e.run(100)
        assert e.finished and 0 < e.stop_round < 100
        mine = assignment_to_values(g, e.assignment()[0])
        assert e.eval_cost(infinity=1000)[1] == 0            # a proper colouring
    want, _, _, info = run_reference_dba(load_dcop_from_file([path]), 100, seed=3, **kw)
    assert info["stop_round"] > 0
    assert got == mine == want
    assert solve(load_dcop_from_file([path]), algo, "adhoc", timeout=20) == want


def test_dba_gpu_refuses_max(pydcop_ready, tmp_path):
    from pydcop.algorithms import AlgorithmDef, ComputationDef
    from pydcop.computations_graph import constraints_hypergraph as chg
    from pydcop.dcop.yamldcop import load_dcop_from_file
    dcop = load_dcop_from_file([hard_coloring_yaml(tmp_path / "hard_max.yaml", "max")])
    algo = AlgorithmDef.build_with_default_param("dba_gpu", {}, mode="max")
    node = chg.build_computation_graph(dcop).nodes[0]
    with pytest.raises(ValueError, match="satisfaction"):
        pydcop_ready.build_computation(ComputationDef(node, algo))


def test_footprint_and_load_like_the_reference(pydcop_ready, tmp_path):
    from pydcop.algorithms import load_algorithm_module
    from pydcop.computations_graph import constraints_hypergraph as chg
    from pydcop.dcop.yamldcop import load_dcop_from_file
    ref, mod = load_algorithm_module("dba"), pydcop_ready
    cg = chg.build_computation_graph(load_dcop_from_file([hard_coloring_yaml(tmp_path / "hard.yaml")]))
    for node in cg.nodes:
        assert mod.computation_memory(node) == ref.computation_memory(node) == len(node.neighbors) * ref.UNIT_SIZE
        for other in node.neighbors:
            assert mod.communication_load(node, other) == ref.communication_load(node, other)


def test_api_runs_dba(pydcop_ready, tmp_path, capsys):
    """`python -m pydcop_amd.api -a dba -p infinity:1000 -p max_distance:3` on a YAML DCOP."""
    from pydcop_amd import api
    api.main(["-a", "dba", "-c", "100", "-p", "infinity:1000", "-p", "max_distance:3", "-p", "seed:3",
              hard_coloring_yaml(tmp_path / "hard.yaml")])
    out = json.loads(capsys.readouterr().out)
    assert out["status"] == "FINISHED" and 0 < out["cycle"] < 100 and out["cost"] == 0
    assert set(out["assignment"]) == {f"v{i}" for i in range(1, 9)}
