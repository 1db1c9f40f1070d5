"""DBA (pydcop/algorithms/dba.py) on the GPU: the ctypes binding of the `mxs_dba_*` entry points
(include/maxsum_gpu.h; device code: pydcop_amd/csrc/dba.h) on the same FlatGraph as the other
engines -- factors are the constraints, variables the DBA computations.  No CPU fallback."""
import ctypes as C
from typing import Optional, Tuple

import numpy as np

from ._binding import EngineBinding
from .engine import load_library
from .graph import FlatGraph, Params
from .mgm import name_ranks

INFINITY = 10000            # the reference's defaults (dba.py:265-268)
MAX_DISTANCE = 50


class DbaEngine(EngineBinding):
    """>>> eng = DbaEngine(graph, Params(mode="min"), infinity=1000, max_distance=50, seed=0)
    >>> eng.run(30)                                    # up to 30 rounds of (ok, improve)
    >>> eng.finished, eng.stop_round                   # a termination counter reached max_distance
    >>> idx, cost = eng.assignment()

    A table entry >= `infinity` is a violated constraint; nothing else of the tables is looked at.
    `mask_budget`: the most bytes the violation bits may take on the device (0: the library's default);
    an instance past it is refused before anything is allocated."""
    PREFIX = "mxs_dba"
    COUNTER = "rounds"

    def __init__(self, graph: FlatGraph, params: Optional[Params] = None, infinity: float = INFINITY,
                 max_distance: int = MAX_DISTANCE, seed: int = 0, mask_budget: int = 0, device: int = 0,
                 lib_path: Optional[str] = None):
        self.infinity, self.max_distance, self.seed = infinity, int(max_distance), int(seed)
        self._lib = load_library(lib_path)
        self.graph = graph
        self.params = params or Params()
        cg, cp = graph.to_c(), self.params.to_c()
        self._rank = name_ranks(graph.var_names) if graph.var_names else None
        h = C.c_void_p()
        self._check(self._lib.mxs_dba_create(C.byref(cg), C.byref(cp),
                                             None if self._rank is None else self._rank.ctypes.data,
                                             float(infinity), self.max_distance, self.seed & (2 ** 64 - 1),
                                             int(mask_budget), int(device), C.byref(h)))
        self._h = h

    def reset(self):
        self._call("reset")

    def run(self, n_rounds: int):
        """`n_rounds` more rounds, or as many as it takes to stop; after a stop, nothing."""
        self._call("run", int(n_rounds))

    def state(self) -> dict:
        """idx, cost (held; has_cost 0: still None), eval, improve, new (-1: still None), counter, consistent"""
        n = self.graph.n_vars
        i32 = lambda: np.empty(n, dtype=np.int32)   # noqa: E731
        out = {"idx": i32(), "cost": i32(), "has_cost": np.empty(n, dtype=np.uint8), "eval": i32(), "improve": i32(),
               "new": i32(), "counter": i32(), "consistent": np.empty(n, dtype=np.uint8)}
        self._call("get_state", *[a.ctypes.data for a in out.values()])
        return out

    def assignment(self) -> Tuple[np.ndarray, np.ndarray]:
        s = self.state()
        return s["idx"], s["cost"].astype(np.float64)

    def weights(self) -> np.ndarray:
        """The weight of every slot = var_rowptr[v] + k (variable v, its k-th constraint)."""
        out = np.empty(len(self.graph.var_edges), dtype=np.int32)
        self._call("get_weights", out.ctypes.data)
        return out

    def _finished(self):
        stopped, at = C.c_int32(0), C.c_int64(0)
        self._call("finished", C.byref(stopped), C.byref(at))
        return bool(stopped.value), int(at.value)

    @property
    def finished(self) -> bool:
        return self._finished()[0]

    @property
    def stop_round(self) -> int:
        """The round in which a stop condition held (0: none yet)."""
        return self._finished()[1]

    @property
    def mask_bytes(self) -> int:
        n = C.c_int64(0)
        self._call("mask_bytes", C.byref(n))
        return int(n.value)
