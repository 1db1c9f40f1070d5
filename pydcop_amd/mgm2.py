"""MGM-2 (pydcop/algorithms/mgm2.py) on the GPU: the ctypes binding of the `mxs_mgm2_*` entry points
(include/maxsum_gpu.h; device code: pydcop_amd/csrc/mgm2.h) on the same FlatGraph as the other
engines -- factors are the constraints, variables the MGM-2 computations.  No CPU fallback."""
import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from ._binding import ReplicaBinding
from .engine import load_library
from .graph import FlatGraph, Params
from .mgm import name_ranks

FAVORS = ("unilateral", "no", "coordinated")
REPLICA_SYMBOLS = ("mxs_mgm2_create_replicas", "mxs_mgm2_replicas", "mxs_mgm2_get_state_replica",
                   "mxs_mgm2_replica_costs", "mxs_mgm2_best_replica")


def check_params(threshold, favor):
    """The reference's parameter definitions (mgm2.py:142-146): `threshold` a float in [0, 1] (the
    probability of being an offerer), `favor` one of unilateral / no / coordinated."""
    try:
        threshold = float(threshold)
    except (TypeError, ValueError):
        raise ValueError(f"Invalid value for parameter threshold: {threshold!r} (float expected)")
    if not 0.0 <= threshold <= 1.0:
        raise ValueError(f"Invalid value for parameter threshold: {threshold} (must be between 0 and 1)")
    if favor not in FAVORS:
        raise ValueError(f"Invalid value for parameter favor: {favor!r} (one of {list(FAVORS)})")
    return threshold, FAVORS.index(favor)


class Mgm2Engine(ReplicaBinding):
    """>>> eng = Mgm2Engine(graph, Params(mode="min"), threshold=0.5, favor="unilateral", seed=0)
    >>> eng.run(30)                                    # 30 rounds (= the reference's stop_cycle 31)
    >>> idx, cost = eng.assignment()

    `replicas=R`: R seeded runs of the instance in one engine (seeds `seed + r` modulo 2**64, or `seeds`), advanced
    by the five launches of one round over one copy of the tables; replica r is bit for bit the engine with that
    seed.  MGM-2's sum stops improving at a local optimum: run it from many seeds and keep the best.
    >>> eng = Mgm2Engine(graph, favor="coordinated", replicas=8, seed=5)
    >>> eng.run(30)
    >>> eng.best(infinity=10000)                       # the best replica's current state
    `replicas=1` without `seeds` is the single run (`mxs_mgm2_create`: the same engine with one replica, launched
    through the single-run kernels)."""
    PREFIX = "mxs_mgm2"
    COUNTER = "rounds"
    STATE_FIELDS = (("idx", np.int32), ("cost", np.float64), ("has_cost", np.uint8))
    REPLICA_SYMBOLS = REPLICA_SYMBOLS
    REPLICA_FEATURE = "MGM-2's replicas"

    def __init__(self, graph: FlatGraph, params: Optional[Params] = None, threshold: float = 0.5,
                 favor: str = "unilateral", seed: int = 0, device: int = 0, lib_path: Optional[str] = None,
                 seeds: Optional[Sequence[int]] = None, replicas: int = 1):
        self.threshold, favor_code = check_params(threshold, favor)
        self.favor, self.seed = favor, int(seed)
        single = seeds is None and int(replicas) == 1
        sd = self._set_seeds(seed, seeds, replicas)     # (no seeds at all: the library refuses 0 replicas)
        self._lib = load_library(lib_path)
        self.graph = graph
        self.params = params or Params()
        cg, cp = graph.to_c(), self.params.to_c()
        self._rank = name_ranks(graph.var_names) if graph.var_names else None
        rank = None if self._rank is None else self._rank.ctypes.data
        h = C.c_void_p()
        if single:
            self._check(self._lib.mxs_mgm2_create(C.byref(cg), C.byref(cp), rank, self.threshold, favor_code,
                                                  self.seed & (2 ** 64 - 1), int(device), C.byref(h)))
        else:
            self._need_replica_symbols("replicas / seeds need them")
            self._check(self._lib.mxs_mgm2_create_replicas(C.byref(cg), C.byref(cp), rank, self.threshold, favor_code,
                                                           sd.ctypes.data, self.replicas, int(device), C.byref(h)))
        self._h = h

    def reset(self):
        self._call("reset")

    def run(self, n_rounds: int):
        self._call("run", int(n_rounds))

    def replica_costs(self, infinity: float = float("inf")) -> Tuple[np.ndarray, np.ndarray]:
        self._need_replica_symbols("replica_costs needs them")
        return super().replica_costs(infinity)

    def best(self, infinity: float = float("inf")) -> Dict:
        """The best replica's current state -- fewest violations, then best cost, then lowest index, ranked on the
        device: {"replica", "cost", "violations", "idx"}."""
        self._need_replica_symbols("best needs them")
        return self._best_ranked(infinity)
