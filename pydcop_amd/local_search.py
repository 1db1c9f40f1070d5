"""What the plug-ins of the local-search family share (pydcop_amd/algorithms/{dsa,mgm,mgm2,gdba,dba}_gpu.py; dpop_gpu
takes the factory of its computations from here too): how the reference's constraints hypergraph is compiled, the
session and the engine adapter their own ones derive from, and the computation class with its `build_computation`.  It
lives outside pydcop_amd/algorithms/ because every file there is on `pydcop.algorithms.__path__` and would be listed as
an algorithm.  The proxies and the session underneath are those of `maxsum_gpu`.
"""
from types import SimpleNamespace

from pydcop_amd.algorithms import maxsum_gpu as _base
from pydcop_amd.compile import compile_nodes
from pydcop_amd.graph import Params


def compile_dcop_for_local_search(dcop):
    """A DCOP compiled as these plug-ins compile it: the nodes of the reference's constraints
    hypergraph by name, each variable's constraints in the node's order."""
    from pydcop.computations_graph import constraints_hypergraph as chg
    cg = chg.build_computation_graph(dcop)
    return _compile_hypergraph(list(cg.nodes))


def _compile_hypergraph(nodes):
    nodes = sorted(nodes, key=lambda n: n.name)
    constraints = {}
    for n in nodes:
        for c in n.constraints:
            constraints.setdefault(c.name, c)
    fac_nodes = [SimpleNamespace(name=name, factor=constraints[name]) for name in sorted(constraints)]
    var_nodes = [SimpleNamespace(name=n.name, variable=n.variable,
                                 links=[SimpleNamespace(factor_node=c.name) for c in n.constraints])
                 for n in nodes]
    return compile_nodes(var_nodes, fac_nodes, noise=0.0)


class EngineAdapter:
    """An engine of the family behind the surface the session drives.  `many`: the engine runs several replicas and
    the best one's values are reported.  A run that can end by itself overrides `quiescent`."""
    FIRST_CYCLE = 0            # 1 where the reference's cycle counter starts at 1
    quiescent = False

    def __init__(self, graph, engine, many=False):
        self.graph, self._e, self._many = graph, engine, many

    def run(self, n: int):
        self._e.run(int(n))

    def assignment(self):
        if not self._many:
            return self._e.assignment()
        return self._e.assignment(self._e.best()["replica"])     # the best replica's values and held costs

    @property
    def cycle_count(self) -> int:
        return self._e.cycle_count + self.FIRST_CYCLE

    def close(self):
        self._e.close()


class LocalSearchSession(_base._Session):
    """The session of maxsum_gpu over the constraints hypergraph: a subclass names its ALGO and its ENGINE (the
    adapter, created with the graph, the Params and the algorithm's parameters)."""
    ENGINE = None

    def _compile_graph(self, p):
        return _compile_hypergraph(cd.node for cd in self.comp_defs.values())

    def _engine_params(self, algo, p):
        return Params(mode=algo.mode, dtype=p["precision"])

    def _make_engine(self, params, p):
        return self.ENGINE(self.graph, params, p)

    def _cycles_to_run(self, p) -> int:
        """`stop_cycle: n` = n - 1 rounds: the reference's cycle counter starts at 1"""
        stop = int(p["stop_cycle"])
        if stop == 1:          # the reference finishes before the first exchange of values
            self.done = True
        return max(0, stop - 1)

    def update_factor(self, name, old, fn):
        raise ValueError(self.ALGO + ": change_factor_function is a maxsum_gpu feature")


def computation_for(algo, name, doc, computation_memory, node_type="VariableComputationNode", check=None):
    """-> (the computation class `name` of the plug-in `algo`: maxsum_gpu's variable proxy with the plug-in's own
    footprint; the plug-in's `build_computation`, which refuses another node type and whatever `check(comp_def)` does)"""
    cls = type(name, (_base.MaxSumGpuVariableComputation,), {
        "__doc__": doc, "__module__": "pydcop_amd.algorithms." + algo,
        "footprint": lambda self: computation_memory(self.computation_def.node)})

    def build_computation(comp_def):
        if comp_def.node.type != node_type:
            raise ValueError(algo + ": unsupported computation node type " + str(comp_def.node.type))
        if check is not None:
            check(comp_def)
        return cls(comp_def)
    return cls, build_computation
