"""mgm_gpu -- the reference's MGM (pydcop/algorithms/mgm.py) on the GPU, behind the algorithm-module
contract (same GRAPH_TYPE `constraints_hypergraph`, the same two parameters with the same defaults,
the same footprint / load formulas), reusing the proxies and the session of `maxsum_gpu`.

One round of MGM = two launches over all variables (pydcop_amd/csrc/mgm.hip).  `stop_cycle: n`
ends like the reference does: after n - 1 rounds (its cycle counter starts at 1, mgm.py:407-411);
0 = keep going, `chunk` rounds per report, until the orchestrator's timeout.  The reference's draws
from the unseeded `random` module are fixed: first domain value at start (unless the variable has
an initial value), first of equally good values; ties between equal gains by name (the
reference's `break_mode: random` never triggers -- mgm.py:543 compares the string with the module
-- so both modes are lexic, here as there).

Extra parameters: `draws: keyed` (default `fixed`) takes the two draws from a counter-based generator keyed on (`seed`,
variable, cycle, draw) instead -- draw 10 the start value of a variable without initial value, draw 11 one of the
equally good values when the gain improves --: a run is reproducible, and bit for bit the reference's own
MgmComputation under the same generator.  The variable index in the keys is the module's compile order: the variables
sorted by name.  `restarts: R` (default 1; needs `draws: keyed`) runs R seeded replicas (seeds seed .. seed + R - 1) in
the one engine and publishes the best replica's values -- fewest entries equal to infinity, then the best solution
cost, evaluated on the device.  MGM's own sum never rises, so a replica's final state is its best: there is no
`best_every`.  The ranking takes no `infinity` (the module has no such parameter: every table entry, however large, is
a cost).  With the defaults the module is the single fixed-draw run above.
"""
from pydcop.algorithms import AlgoParameterDef

from pydcop_amd.algorithms import maxsum_gpu as _base
from pydcop_amd.local_search import EngineAdapter, LocalSearchSession, computation_for

GRAPH_TYPE = "constraints_hypergraph"
HEADER_SIZE = 100
UNIT_SIZE = 5

algo_params = [
    AlgoParameterDef("break_mode", "str", ["lexic", "random"], "lexic"),
    AlgoParameterDef("stop_cycle", "int", None, 0),
    AlgoParameterDef("precision", "str", ["f64", "f32"], "f64"),
    AlgoParameterDef("chunk", "int", None, 10),
    AlgoParameterDef("draws", "str", ["fixed", "keyed"], "fixed"),
    AlgoParameterDef("seed", "int", None, 0),
    AlgoParameterDef("restarts", "int", None, 1),
]


def computation_memory(computation) -> float:
    """pydcop/algorithms/mgm.py:82-112: one value per neighbour."""
    neighbors = set(n for link in computation.links for n in link.nodes if n not in computation.name)
    return len(neighbors) * UNIT_SIZE


def communication_load(src, target: str) -> float:
    """pydcop/algorithms/mgm.py:115-135."""
    return UNIT_SIZE + HEADER_SIZE


class _RoundEngine(EngineAdapter):
    """MgmEngine behind the surface the session drives."""
    FIRST_CYCLE = 1          # the reference's counter starts at 1 (mgm.py:407)

    def __init__(self, graph, params, p):
        from pydcop_amd.mgm import MgmEngine
        many = int(p["restarts"]) > 1
        if p["draws"] == "fixed":
            if many:
                raise ValueError("mgm_gpu: restarts needs draws:keyed (with the fixed draws every run is the same run)")
            engine = MgmEngine(graph, params)
        else:
            engine = MgmEngine(graph, params, draws=p["draws"], seed=int(p["seed"]), replicas=int(p["restarts"]))
        super().__init__(graph, engine, many)


class _MgmSession(LocalSearchSession):
    ALGO, ENGINE = "mgm_gpu", _RoundEngine


_base.SESSION_CLASSES["mgm_gpu"] = _MgmSession
MgmGpuComputation, build_computation = computation_for(
    "mgm_gpu", "MgmGpuComputation", "Stands for an MgmComputation (pydcop/algorithms/mgm.py:213).", computation_memory)
