"""mgm2_gpu -- the reference's MGM-2 (pydcop/algorithms/mgm2.py) on the GPU, behind the algorithm-module
contract (same GRAPH_TYPE `constraints_hypergraph`, the same three parameters with the same defaults,
the same footprint / load formulas), reusing the proxies and the session of `maxsum_gpu`.

One round of MGM-2 = five launches over all variables (pydcop_amd/csrc/mgm2.h).  `stop_cycle: n` ends
like the reference does: after n - 1 rounds (`_send_value` counts the cycle before it tests for the
stop, mgm2.py:659-672); 0 = keep going, `chunk` rounds per report, until the orchestrator's timeout.
Extra parameter `seed` (default 0): every stochastic choice -- start value, offerer test, partner,
best unilateral value, the `favor: no` coin, the accepted offer -- comes from the counter-based
generator of dsa_gpu keyed on (seed, variable, round, draw) over canonically ordered sequences, where
the reference draws from Python's unseeded `random`: a run is reproducible, and bit for bit the
reference's own Mgm2Computation under the same generator.  `restarts: R` (default 1) runs R seeded replicas (seeds
seed .. seed + R - 1) in the one engine and publishes the best replica's values and held costs -- fewest entries equal
to infinity, then the best solution cost, evaluated on the device; the ranking takes no `infinity` (the module has no
such parameter: every table entry, however large, is a cost).  With the defaults the module is the single run above.
"""
from pydcop.algorithms import AlgoParameterDef

from pydcop_amd.algorithms import maxsum_gpu as _base
from pydcop_amd.local_search import (EngineAdapter, LocalSearchSession, compile_dcop_for_local_search,  # noqa: F401
                                     computation_for)                          # (compile_dcop_...: importable from here)

GRAPH_TYPE = "constraints_hypergraph"
HEADER_SIZE = 100
UNIT_SIZE = 5

algo_params = [
    AlgoParameterDef("threshold", "float", None, 0.5),
    AlgoParameterDef("favor", "str", ["unilateral", "no", "coordinated"], "unilateral"),
    AlgoParameterDef("stop_cycle", "int", None, 0),
    AlgoParameterDef("precision", "str", ["f64", "f32"], "f64"),
    AlgoParameterDef("seed", "int", None, 0),
    AlgoParameterDef("chunk", "int", None, 10),
    AlgoParameterDef("restarts", "int", None, 1),
]


def computation_memory(computation) -> float:
    """pydcop/algorithms/mgm2.py:66-91: a value and a gain per neighbour."""
    neighbors = set(n for link in computation.links for n in link.nodes if n not in computation.name)
    return len(neighbors) * 2 * UNIT_SIZE


def communication_load(src, target: str) -> float:
    """pydcop/algorithms/mgm2.py:94-128: the offer message, (two values and a gain) per pair of values."""
    target_v = None
    for c in src.constraints:
        for v in c.dimensions:
            if v.name == target:
                target_v = v
    if not target_v:
        raise ValueError("target variable {} not found in constraints for {}".format(target, src))
    nb_pairs = len(target_v.domain) * len(src.variable.domain)
    return nb_pairs * UNIT_SIZE * 3 + HEADER_SIZE


class _RoundEngine(EngineAdapter):
    """Mgm2Engine behind the surface the session drives."""
    FIRST_CYCLE = 1          # the reference's counter starts at 1 (mgm2.py:659)

    def __init__(self, graph, params, p):
        from pydcop_amd.mgm2 import Mgm2Engine
        super().__init__(graph, Mgm2Engine(graph, params, threshold=p["threshold"], favor=p["favor"], seed=int(p["seed"]),
                                           replicas=int(p["restarts"])), many=int(p["restarts"]) > 1)


class _Mgm2Session(LocalSearchSession):
    ALGO, ENGINE = "mgm2_gpu", _RoundEngine


_base.SESSION_CLASSES["mgm2_gpu"] = _Mgm2Session
Mgm2GpuComputation, build_computation = computation_for(
    "mgm2_gpu", "Mgm2GpuComputation", "Stands for an Mgm2Computation (pydcop/algorithms/mgm2.py:399).", computation_memory)
