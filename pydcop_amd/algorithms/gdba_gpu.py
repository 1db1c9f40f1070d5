"""gdba_gpu -- the reference's GDBA (pydcop/algorithms/gdba.py) on the GPU, behind the algorithm-module
contract (same GRAPH_TYPE `constraints_hypergraph`, the same three parameters with the same choices and
defaults, the same footprint / load formulas), reusing the proxies and the session of `maxsum_gpu`.

One round of GDBA = two launches over all variables (pydcop_amd/csrc/gdba.h).  The reference has no stop
condition (gdba.py:421-422); `stop_cycle: n` ends here as it does for mgm_gpu, after n - 1 rounds (the
cycle counter starts at 1); 0 = keep going, `chunk` rounds per report, until the orchestrator's timeout
or the 65535 rounds the 16-bit modifier counters allow (the run then ends FINISHED, with a warning).  Extra parameter `seed` (default 0): the two
stochastic choices -- start value, one of the best values -- come from the counter-based generator of
dsa_gpu keyed on (seed, variable, round, draw) over domain order, where the reference draws from Python's
unseeded `random`: a run is reproducible, and bit for bit the reference's own GdbaComputation under the
same generator.
"""
from pydcop.algorithms import AlgoParameterDef

from pydcop_amd.algorithms import maxsum_gpu as _base
from pydcop_amd.local_search import EngineAdapter, LocalSearchSession, computation_for

GRAPH_TYPE = "constraints_hypergraph"
HEADER_SIZE = 100
UNIT_SIZE = 5

algo_params = [
    AlgoParameterDef("modifier", "str", ["A", "M"], "A"),
    AlgoParameterDef("violation", "str", ["NZ", "NM", "MX"], "NZ"),
    AlgoParameterDef("increase_mode", "str", ["E", "R", "C", "T"], "E"),
    AlgoParameterDef("stop_cycle", "int", None, 0),
    AlgoParameterDef("precision", "str", ["f64", "f32"], "f64"),
    AlgoParameterDef("seed", "int", None, 0),
    AlgoParameterDef("chunk", "int", None, 10),
]


def computation_memory(computation) -> float:
    """pydcop/algorithms/gdba.py:75-97: one value per neighbour.  The reference's own function walks
    `computation.neighbors` (names) as if they were links and raises AttributeError on a real node; this is the
    formula it states, over the links, as mgm.py:82-112 writes it."""
    neighbors = set(n for link in computation.links for n in link.nodes if n not in computation.name)
    return len(neighbors) * UNIT_SIZE


def communication_load(src, target: str) -> float:
    """pydcop/algorithms/gdba.py:100-123: a value and an improvement."""
    return 2 * UNIT_SIZE + HEADER_SIZE


class _RoundEngine(EngineAdapter):
    """GdbaEngine behind the surface the session drives."""
    FIRST_CYCLE = 1          # the reference's counter starts at 1 (gdba.py:420)

    def __init__(self, graph, params, p):
        from pydcop_amd.gdba import MAX_ROUNDS, GdbaEngine
        self._max = MAX_ROUNDS
        super().__init__(graph, GdbaEngine(graph, params, modifier=p["modifier"], violation=p["violation"],
                                           increase_mode=p["increase_mode"], seed=int(p["seed"])))

    def run(self, n: int):
        left = self._max - self._e.cycle_count
        self._e.run(min(int(n), left))
        if int(n) >= left:
            import logging
            logging.getLogger("pydcop.algo.gdba_gpu").warning(
                "gdba_gpu: %d rounds done, the range of the 16-bit modifier counters: the run ends here", self._max)

    @property
    def quiescent(self) -> bool:
        """the session ends a `stop_cycle: 0` run (status FINISHED) once no further round can be run"""
        return self._e.cycle_count >= self._max


class _GdbaSession(LocalSearchSession):
    ALGO, ENGINE = "gdba_gpu", _RoundEngine


_base.SESSION_CLASSES["gdba_gpu"] = _GdbaSession
GdbaGpuComputation, build_computation = computation_for(
    "gdba_gpu", "GdbaGpuComputation", "Stands for a GdbaComputation (pydcop/algorithms/gdba.py:189).", computation_memory)
