"""dsa_gpu -- the reference's DSA (pydcop/algorithms/dsa.py, variants A / B / C) on the GPU, behind
the algorithm-module contract (same GRAPH_TYPE `constraints_hypergraph`, the same four parameters
with the same defaults, the same footprint / load formulas), reusing the proxies and the session of
`maxsum_gpu`.

One cycle of DSA = one launch over all variables (pydcop_amd/csrc/dsa.hip).  `stop_cycle: n` ends
after n cycles like the reference (dsa.py:351-354); 0 = keep going, `chunk` cycles per report, until
the orchestrator's timeout.  Extra parameter `seed` (default 0): every stochastic choice -- initial
value, move test, choice among equally good values -- comes from a counter-based generator keyed on
(seed, variable, cycle, draw), where the reference draws from Python's unseeded `random`: a run is
reproducible, and bit for bit the reference's own DsaComputation under the same generator.

`restarts: R` (default 1) runs R seeded replicas (seeds seed .. seed + R - 1) in the one engine and reports the
best replica's values -- fewest entries equal to infinity, then the best solution cost, evaluated on the device;
`best_every: k` (default 0: off) keeps every replica's best state seen at cycle 0 and after every k-th cycle and
reports the best record instead of the best final state.  With the defaults the module is the single run above.
The ranking takes no `infinity`: the module has no such parameter (the orchestrator applies its own to the values it
collects), so every table entry, however large, is a cost and the replicas are ranked by the plain sum
(`solve_dcop` / `solve_flat` rank with the caller's infinity).  The cost published beside a value is the one the
replica's computation HOLDS NOW (dsa.py: the cost of its last move): with `best_every` the values are a snapshot of
an earlier cycle, the held costs are still the current ones -- the engine keeps no snapshot of them.
"""
from pydcop.algorithms import AlgoParameterDef

from pydcop_amd.algorithms import maxsum_gpu as _base
from pydcop_amd.local_search import EngineAdapter, LocalSearchSession, computation_for

GRAPH_TYPE = "constraints_hypergraph"
HEADER_SIZE = 0
UNIT_SIZE = 1

algo_params = [
    AlgoParameterDef("probability", "float", None, 0.7),
    AlgoParameterDef("p_mode", "str", ["fixed", "arity"], "fixed"),
    AlgoParameterDef("variant", "str", ["A", "B", "C"], "B"),
    AlgoParameterDef("stop_cycle", "int", None, 0),
    AlgoParameterDef("precision", "str", ["f64", "f32"], "f64"),
    AlgoParameterDef("seed", "int", None, 0),
    AlgoParameterDef("chunk", "int", None, 10),
    AlgoParameterDef("restarts", "int", None, 1),
    AlgoParameterDef("best_every", "int", None, 0),
]


def computation_memory(computation) -> float:
    """pydcop/algorithms/dsa.py:138-158: one value per neighbour."""
    neighbors = set(n for link in computation.links for n in link.nodes if n not in computation.name)
    return len(neighbors) * UNIT_SIZE


def communication_load(src, target: str) -> float:
    """pydcop/algorithms/dsa.py:161-183."""
    return UNIT_SIZE + HEADER_SIZE


class _CycleEngine(EngineAdapter):
    """DsaEngine behind the surface the session drives."""

    def __init__(self, graph, params, p):
        from pydcop_amd.dsa import DsaEngine
        super().__init__(graph, DsaEngine(graph, params, variant=p["variant"], probability=float(p["probability"]),
                                          p_mode=p["p_mode"], seed=int(p["seed"]), replicas=int(p["restarts"])),
                         many=int(p["restarts"]) > 1 or int(p["best_every"]) > 0)
        if self._many:
            self._e.track_best(int(p["best_every"]), float("inf"))

    def assignment(self):
        if not self._many:
            return self._e.assignment()
        best = self._e.best()               # the best replica: its record (best_every > 0) or its state
        return best["idx"], self._e.assignment(best["replica"])[1]   # (held costs: the current ones, see above)


class _DsaSession(LocalSearchSession):
    ALGO, ENGINE = "dsa_gpu", _CycleEngine

    def _cycles_to_run(self, p) -> int:
        return int(p["stop_cycle"])


_base.SESSION_CLASSES["dsa_gpu"] = _DsaSession
DsaGpuComputation, build_computation = computation_for(
    "dsa_gpu", "DsaGpuComputation", "Stands for a DsaComputation (pydcop/algorithms/dsa.py:214).", computation_memory)
