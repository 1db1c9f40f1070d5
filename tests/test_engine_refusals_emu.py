"""What the DSA / MGM / MGM-2 / GDBA / DPOP engines share on the host, on the emulated build: the graphs every one
of them refuses (with the same text), the assignment `eval_cost` refuses, and `eval_cost` itself against a direct
numpy evaluation.  One small graph: x0 (2 values), x1 (3), x2 (2); a binary constraint over (x0, x1), a unary
one over x2."""
import numpy as np
import pytest

from pydcop_amd.engine import MaxSumGpuError
from pydcop_amd.graph import FlatGraph, Params

BIG = 1000.0  # the `infinity` of eval_cost: finite, MGM-2 / GDBA / DPOP take no inf / NaN entries
ENGINES = ("dsa", "mgm", "mgm2", "gdba", "dpop")
USES_INIT_IDX = ("mgm", "mgm2", "gdba")  # DSA and DPOP never read init_idx


def small_graph():
    edge_var = np.array([0, 1, 2], dtype=np.int32)
    vrow, vedges = FlatGraph.var_side_from_edges(edge_var, 3)
    tables = np.array([1, 2, 3, 4, BIG, 6, 7, 8], dtype=np.float64)   # [x0][x1] row-major, then [x2]
    var_cost = np.array([0.5, 0.25, 0, BIG, 1, 2, 0.125], dtype=np.float64)
    return FlatGraph(dom_size=[2, 3, 2], var_cost=var_cost, factor_rowptr=[0, 2, 3], edge_var=edge_var,
                     table_off=[0, 6, 8], tables=tables, var_rowptr=vrow, var_edges=vedges,
                     init_idx=np.array([1, 2, 0], dtype=np.int32)).validate()


def make(engine, graph, lib):
    if engine == "dsa":
        from pydcop_amd.dsa import DsaEngine
        return DsaEngine(graph, Params(), lib_path=lib)
    if engine == "mgm":
        from pydcop_amd.mgm import MgmEngine
        return MgmEngine(graph, Params(), lib_path=lib)
    if engine == "mgm2":
        from pydcop_amd.mgm2 import Mgm2Engine
        return Mgm2Engine(graph, Params(), lib_path=lib)
    if engine == "gdba":
        from pydcop_amd.gdba import GdbaEngine
        return GdbaEngine(graph, Params(), lib_path=lib)
    from pydcop_amd.dpop import DpopEngine, pack_tree
    return DpopEngine(graph, Params(), tree=pack_tree([-1, 0, 1], [[1], [2], []]), lib_path=lib)  # the chain x0 - x1 - x2


@pytest.fixture(scope="module")
def emu_lib():
    from emu.build_emu import build
    return build()


# One corrupted array at a time.  FlatGraph.to_c() and the bindings check nothing of the arrays' contents, so
# every case reaches the library.
def _empty_domain(g):
    g.dom_size[1] = 0


def _factor_without_variable(g):
    g.factor_rowptr[1] = 3   # the first constraint takes all three edges, the second is left with none


def _edge_var_out_of_range(g):
    g.edge_var[2] = g.n_vars


def _init_idx_out_of_the_domain(g):
    g.init_idx[1] = g.dom_size[1]


REFUSED = [(_empty_domain, "empty domain"), (_factor_without_variable, "factor without variable"),
           (_edge_var_out_of_range, "edge_var out of range"), (_init_idx_out_of_the_domain, "init_idx out of the domain")]


@pytest.mark.parametrize("engine", ENGINES)
def test_valid_graph_is_accepted(engine, emu_lib):
    make(engine, small_graph(), emu_lib).close()


@pytest.mark.parametrize("corrupt,message", REFUSED, ids=lambda x: x if isinstance(x, str) else "")
@pytest.mark.parametrize("engine", ENGINES)
def test_refused_graph(engine, corrupt, message, emu_lib):
    g = small_graph()
    corrupt(g)
    if message.startswith("init_idx") and engine not in USES_INIT_IDX:
        make(engine, g, emu_lib).close()   # the array is never read: the graph is taken
        return
    with pytest.raises(MaxSumGpuError) as err:
        make(engine, g, emu_lib)
    assert str(err.value) == f"maxsum_gpu error -1: {message}"


@pytest.mark.parametrize("engine", ENGINES)
def test_refused_assignment(engine, emu_lib):
    with make(engine, small_graph(), emu_lib) as e:
        for idx in ([0, 3, 0], [0, -1, 0], [0, 0, 2]):
            with pytest.raises(MaxSumGpuError) as err:
                e.eval_cost(idx, infinity=BIG)
            assert str(err.value) == "maxsum_gpu error -1: assignment index out of the domain"


def numpy_cost(g, idx, infinity):
    terms = [g.tables[:6].reshape(2, 3)[idx[0], idx[1]], g.tables[6:][idx[2]]]
    terms += [g.var_cost[g.cost_off[v] + idx[v]] for v in range(3)]
    soft = 0.0
    for t in terms:
        if t != infinity:
            soft += t
    return soft, sum(1 for t in terms if t == infinity)


@pytest.mark.parametrize("idx", [[1, 1, 0], [0, 2, 1], [1, 0, 1], [0, 0, 0]], ids=str)
def test_eval_cost_agrees(idx, emu_lib):
    """[1, 1, 0] meets both the table entry and the variable cost that equal `infinity`."""
    g = small_graph()
    want = numpy_cost(g, idx, BIG)
    if idx == [1, 1, 0]:
        assert want == (7 + 0.25 + 2, 2)
    for engine in ENGINES:
        with make(engine, g, emu_lib) as e:
            assert e.eval_cost(idx, infinity=BIG) == want, engine
            # (with another `infinity` nothing is a violation)
            assert e.eval_cost(idx, infinity=float("inf")) == numpy_cost(g, idx, float("inf")), engine
