"""dpop_gpu -- the reference's DPOP (pydcop/algorithms/dpop.py) on the GPU, behind the algorithm-module
contract: the same GRAPH_TYPE `pseudotree`, no algorithm parameter of the reference's (it defines none),
`computation_memory` / `communication_load` raising NotImplementedError like the reference's.

The session takes parent and children order from every node's links (`get_dfs_relations`), compiles the
nodes' constraints in node order (the engine gives each constraint to the lowest node of its scope, as
dpop.py:188-199 does), solves once -- UTIL bottom-up, VALUE top-down, pydcop_amd/csrc/dpop.h -- and every
proxy computation then selects its value with the cost its DpopAlgo would report, and finishes.
Extra parameters: `precision` (f64 | f32) and `max_bytes` (the budget of the UTIL tables; 0 = a share of
the free device memory): an instance whose tables do not fit is refused with the bytes it needs.
"""
from pydcop.algorithms import AlgoParameterDef
from pydcop.computations_graph.pseudotree import get_dfs_relations
from pydcop.infrastructure.computations import ComputationException

from pydcop_amd.algorithms import maxsum_gpu as _base
from pydcop_amd.graph import Params
from pydcop_amd.local_search import _compile_hypergraph, computation_for

GRAPH_TYPE = "pseudotree"

algo_params = [
    AlgoParameterDef("precision", "str", ["f64", "f32"], "f64"),
    AlgoParameterDef("max_bytes", "int", None, 0),
]


def computation_memory(*args):
    raise NotImplementedError("DPOP has no computation memory implementation (yet)")


def communication_load(*args):
    raise NotImplementedError("DPOP has no communication_load implementation (yet)")


def compile_pseudotree(nodes):
    """PseudoTreeNodes -> (FlatGraph, (parent, child_rowptr, child_idx)): variables by name, every
    variable's constraints in its node's order, the tree as the nodes' links give it."""
    from pydcop_amd.dpop import pack_tree
    nodes = sorted(nodes, key=lambda n: n.name)
    graph = _compile_hypergraph(nodes)       # (a pseudo-tree node has the name, variable and constraints it reads)
    index = {name: i for i, name in enumerate(graph.var_names)}
    parent, children = [-1] * len(nodes), [[] for _ in nodes]
    for n in nodes:
        p, _, ch, _ = get_dfs_relations(n)
        parent[index[n.name]] = -1 if p is None else index[p]
        children[index[n.name]] = [index[c] for c in ch]
    return graph, pack_tree(parent, children)


class _SolvedEngine:
    """DpopEngine behind the surface the session drives: solved when it is created, no cycles."""
    cycle_count = 0

    def __init__(self, graph, params, tree, max_bytes):
        from pydcop_amd.dpop import DpopEngine
        self.graph = graph
        self._e = DpopEngine(graph, params, tree=tree, max_bytes=max_bytes)
        self._e.solve()

    def run(self, n: int):
        pass

    def assignment(self):
        return self._e.assignment()

    def close(self):
        self._e.close()


class _DpopSession(_base._Session):
    ALGO = "dpop_gpu"

    def _open(self):
        missing = sorted({n for cd in self.comp_defs.values() for n in cd.node.neighbors} - set(self.comp_defs))
        if missing:
            raise ComputationException("dpop_gpu needs every computation of the pseudo-tree in one process "
                                       "(thread mode); not deployed here: " + ", ".join(missing[:8]))
        algo = next(iter(self.comp_defs.values())).algo
        self.graph, tree = compile_pseudotree(cd.node for cd in self.comp_defs.values())
        self.var_index = {n: i for i, n in enumerate(self.graph.var_names)}
        self.engine = _SolvedEngine(self.graph, Params(mode=algo.mode, dtype=algo.params["precision"]), tree,
                                    int(algo.params["max_bytes"]))
        self.stop_cycle, self.chunk = 1, 1       # (advance(): one no-op run, then every proxy finishes)
        self._fetch()

    def update_factor(self, name, old, fn):
        raise ValueError("dpop_gpu: change_factor_function is a maxsum_gpu feature")


_base.SESSION_CLASSES["dpop_gpu"] = _DpopSession
DpopGpuComputation, build_computation = computation_for(
    "dpop_gpu", "DpopGpuComputation", "Stands for a DpopAlgo (pydcop/algorithms/dpop.py:115).", computation_memory,
    node_type="PseudoTreeComputation")
