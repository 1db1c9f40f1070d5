"""MGM (pydcop/algorithms/mgm.py) on the GPU: the ctypes binding of the `mxs_mgm_*` entry points
(include/maxsum_gpu.h; device code: pydcop_amd/csrc/mgm.hip) on the same FlatGraph as the Max-Sum
engine -- factors are the constraints, variables the MGM computations.  No CPU fallback."""
import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from ._binding import ReplicaBinding
from .engine import load_library
from .graph import FlatGraph, Params

DRAWS = ("fixed", "keyed")
KEYED_SYMBOLS = ("mxs_mgm_create_keyed", "mxs_mgm_replicas", "mxs_mgm_get_state_replica", "mxs_mgm_replica_costs",
                 "mxs_mgm_best_replica")


def name_ranks(names) -> np.ndarray:
    """Rank of every variable's name in sorted order: MGM breaks ties with `sorted(names)`
    (mgm.py:566-575)."""
    order = sorted(range(len(names)), key=lambda i: names[i])
    rank = np.empty(len(names), dtype=np.int32)
    rank[order] = np.arange(len(names), dtype=np.int32)
    return rank


class MgmEngine(ReplicaBinding):
    """>>> eng = MgmEngine(graph, Params(mode="min"))   # every computation started
    >>> eng.run(30)                                    # 30 rounds (= the reference's stop_cycle 31)
    >>> idx, cost = eng.assignment()

    `draws="fixed"` (the default) fixes the reference's two draws from the unseeded `random`: first domain value at
    start, first of equally good values.  `draws="keyed"` takes them from the counter-based generator DSA uses, keyed
    on (seed, variable, cycle, draw): draw 10 the start value of a variable that has no initial value, draw 11 one of
    the best values when the gain improves.  `replicas=R` (keyed only): R seeded runs of the instance in one engine
    (seeds `seed + r` modulo 2**64, or `seeds`), advanced by the same launches over one copy of the tables; replica
    r is bit for bit the keyed engine with that seed.  MGM's own sum never rises, so a run's final state is its best.
    >>> eng = MgmEngine(graph, draws="keyed", replicas=8, seed=5)
    >>> eng.run(30)
    >>> eng.best(infinity=10000)                       # the best replica's final state
    """
    PREFIX = "mxs_mgm"
    COUNTER = "rounds"
    STATE_FIELDS = (("idx", np.int32), ("cost", np.float64), ("has_cost", np.uint8), ("gain", np.float64),
                    ("new", np.int32))
    REPLICA_SYMBOLS = KEYED_SYMBOLS
    REPLICA_FEATURE = "MGM's keyed draws"

    def __init__(self, graph: FlatGraph, params: Optional[Params] = None, device: int = 0,
                 lib_path: Optional[str] = None, draws: str = "fixed", seed: int = 0,
                 seeds: Optional[Sequence[int]] = None, replicas: int = 1):
        if draws not in DRAWS:
            raise ValueError(f"Invalid value {draws!r} for parameter draws, must be one of {list(DRAWS)}")
        if draws == "fixed" and (int(replicas) != 1 or seeds is not None):
            raise ValueError("replicas / seeds need draws=\"keyed\": with the fixed draws every run is the same run")
        sd = self._set_seeds(seed, seeds, replicas)
        self._lib = load_library(lib_path)
        self.graph = graph
        self.params = params or Params()
        self.draws = draws
        cg, cp = graph.to_c(), self.params.to_c()
        self._rank = name_ranks(graph.var_names) if graph.var_names else None
        rank = None if self._rank is None else self._rank.ctypes.data
        h = C.c_void_p()
        if draws == "fixed":
            self._check(self._lib.mxs_mgm_create(C.byref(cg), C.byref(cp), rank, int(device), C.byref(h)))
        else:
            self._need_replica_symbols("draws=\"keyed\" needs them")
            self._check(self._lib.mxs_mgm_create_keyed(C.byref(cg), C.byref(cp), rank, sd.ctypes.data, self.replicas,
                                                       int(device), C.byref(h)))
        self._h = h
        self._set_value_rank()

    def reset(self):
        self._call("reset")

    def run(self, n_rounds: int):
        self._call("run", int(n_rounds))

    def _keyed_only(self, what):
        if self.draws != "keyed":
            raise ValueError(f"{what} needs draws=\"keyed\"")

    def replica_costs(self, infinity: float = float("inf")) -> Tuple[np.ndarray, np.ndarray]:
        self._keyed_only("replica_costs")
        return super().replica_costs(infinity)

    def best(self, infinity: float = float("inf")) -> Dict:
        """The best replica's current state -- fewest violations, then best cost, then lowest index, ranked on the
        device: {"replica", "cost", "violations", "idx"}."""
        self._keyed_only("best")
        return self._best_ranked(infinity)
