"""MGM (pydcop/algorithms/mgm.py) on the GPU: the ctypes binding of the `mxs_mgm_*` entry points
(include/maxsum_gpu.h; device code: pydcop_amd/csrc/mgm.hip) on the same FlatGraph as the Max-Sum
engine -- factors are the constraints, variables the MGM computations.  No CPU fallback."""
import ctypes as C
from typing import Optional, Tuple

import numpy as np

from ._binding import EngineBinding
from .engine import load_library
from .graph import FlatGraph, Params


def name_ranks(names) -> np.ndarray:
    """Rank of every variable's name in sorted order: MGM breaks ties with `sorted(names)`
    (mgm.py:566-575)."""
    order = sorted(range(len(names)), key=lambda i: names[i])
    rank = np.empty(len(names), dtype=np.int32)
    rank[order] = np.arange(len(names), dtype=np.int32)
    return rank


class MgmEngine(EngineBinding):
    """>>> eng = MgmEngine(graph, Params(mode="min"))   # every computation started
    >>> eng.run(30)                                    # 30 rounds (= the reference's stop_cycle 31)
    >>> idx, cost = eng.assignment()
    """
    PREFIX = "mxs_mgm"
    COUNTER = "rounds"

    def __init__(self, graph: FlatGraph, params: Optional[Params] = None, device: int = 0,
                 lib_path: Optional[str] = None):
        self._lib = load_library(lib_path)
        self.graph = graph
        self.params = params or Params()
        cg, cp = graph.to_c(), self.params.to_c()
        self._rank = name_ranks(graph.var_names) if graph.var_names else None
        h = C.c_void_p()
        self._check(self._lib.mxs_mgm_create(C.byref(cg), C.byref(cp),
                                             None if self._rank is None else self._rank.ctypes.data,
                                             int(device), C.byref(h)))
        self._h = h
        # cost ties of a variable without neighbours break on the domain VALUE (relations.py:1661-1665):
        # only needed when some domain is not written in ascending order
        self._vrank = graph.value_rank()
        if self._vrank is not None:
            self._call("set_value_rank", self._vrank.ctypes.data)

    def reset(self):
        self._call("reset")

    def run(self, n_rounds: int):
        self._call("run", int(n_rounds))

    def state(self) -> dict:
        n = self.graph.n_vars
        out = {"idx": np.empty(n, dtype=np.int32), "cost": np.empty(n), "has_cost": np.empty(n, dtype=np.uint8),
               "gain": np.empty(n), "new": np.empty(n, dtype=np.int32)}
        self._call("get_state", *[out[k].ctypes.data for k in ("idx", "cost", "has_cost", "gain", "new")])
        return out

    def assignment(self) -> Tuple[np.ndarray, np.ndarray]:
        s = self.state()
        return s["idx"], s["cost"]
