"""DSA (pydcop/algorithms/dsa.py, variants A / B / C) on the GPU: the ctypes binding of the
`mxs_dsa_*` entry points (include/maxsum_gpu.h; device code: pydcop_amd/csrc/dsa.hip) on the same
FlatGraph as the Max-Sum engine.  Every stochastic choice comes from a counter-based generator keyed
on (seed, variable, cycle, draw): a run is reproducible and independent of scheduling.  No CPU
fallback."""
import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from ._binding import ReplicaBinding
from .engine import load_library
from .graph import FlatGraph, Params

VARIANTS = {"A": 0, "B": 1, "C": 2}


class DsaEngine(ReplicaBinding):
    """>>> eng = DsaEngine(graph, Params(mode="min"), variant="B", probability=0.7, seed=1)
    >>> eng.run(30)                                    # 30 cycles (= the reference's stop_cycle 30)
    >>> idx, cost = eng.assignment()

    `replicas=R`: R seeded runs of the instance in one engine (seeds `seed + r` modulo 2**64, or `seeds`),
    advanced by the same launches over one copy of the tables; replica r is bit for bit the engine with that seed.
    >>> eng = DsaEngine(graph, replicas=8, seed=5)
    >>> eng.track_best(every=1, infinity=10000)        # keep every replica's best state on the device
    >>> eng.run(30)
    >>> eng.best()                                     # the best replica's record
    """
    PREFIX = "mxs_dsa"
    COUNTER = "cycles"
    STATE_FIELDS = (("idx", np.int32), ("cost", np.float64))

    def __init__(self, graph: FlatGraph, params: Optional[Params] = None, variant: str = "B",
                 probability: float = 0.7, p_mode: str = "fixed", seed: int = 0, device: int = 0,
                 lib_path: Optional[str] = None, replicas: int = 1, seeds: Optional[Sequence[int]] = None):
        if variant not in VARIANTS:
            raise ValueError(f"Invalid value {variant!r} for parameter variant, must be one of ['A', 'B', 'C']")
        if p_mode not in ("fixed", "arity"):
            raise ValueError(f"Invalid value {p_mode!r} for parameter p_mode, must be one of ['arity', 'fixed']")
        self._lib = load_library(lib_path)
        self.graph = graph
        self.params = params or Params()
        cg, cp = graph.to_c(), self.params.to_c()
        sd = self._set_seeds(seed, seeds, replicas)
        h = C.c_void_p()
        self._check(self._lib.mxs_dsa_create_replicas(C.byref(cg), C.byref(cp), VARIANTS[variant], float(probability),
                                                      1 if p_mode == "arity" else 0, sd.ctypes.data, self.replicas,
                                                      int(device), C.byref(h)))
        self._h = h
        self._set_value_rank()

    def reset(self):
        self._call("reset")

    def run(self, n_cycles: int):
        self._call("run", int(n_cycles))

    def track_best(self, every: int = 1, infinity: float = float("inf")):
        """Keep, per replica, the best state seen at cycle 0 and after every `every`-th cycle (0: off; the
        `infinity` then only serves `best()`).  Clears the records."""
        self._track_best(every, infinity)

    def best(self, replica: int = -1) -> Dict:
        """The record of `replica` (-1: of the best replica: fewest violations, then best cost, then lowest
        index) when tracking is on, else its current state: {"replica", "cycle", "cost", "violations", "idx"}."""
        return self._best_record(replica)
