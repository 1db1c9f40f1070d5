"""DSA (pydcop/algorithms/dsa.py, variants A / B / C) on the GPU: the ctypes binding of the
`mxs_dsa_*` entry points (include/maxsum_gpu.h; device code: pydcop_amd/csrc/dsa.hip) on the same
FlatGraph as the Max-Sum engine.  Every stochastic choice comes from a counter-based generator keyed
on (seed, variable, cycle, draw): a run is reproducible and independent of scheduling.  No CPU
fallback."""
import ctypes as C
from typing import Optional, Tuple

import numpy as np

from ._binding import EngineBinding
from .engine import load_library
from .graph import FlatGraph, Params

VARIANTS = {"A": 0, "B": 1, "C": 2}


class DsaEngine(EngineBinding):
    """>>> eng = DsaEngine(graph, Params(mode="min"), variant="B", probability=0.7, seed=1)
    >>> eng.run(30)                                    # 30 cycles (= the reference's stop_cycle 30)
    >>> idx, cost = eng.assignment()
    """
    PREFIX = "mxs_dsa"
    COUNTER = "cycles"

    def __init__(self, graph: FlatGraph, params: Optional[Params] = None, variant: str = "B",
                 probability: float = 0.7, p_mode: str = "fixed", seed: int = 0, device: int = 0,
                 lib_path: Optional[str] = None):
        if variant not in VARIANTS:
            raise ValueError(f"Invalid value {variant!r} for parameter variant, must be one of ['A', 'B', 'C']")
        if p_mode not in ("fixed", "arity"):
            raise ValueError(f"Invalid value {p_mode!r} for parameter p_mode, must be one of ['arity', 'fixed']")
        self._lib = load_library(lib_path)
        self.graph = graph
        self.params = params or Params()
        cg, cp = graph.to_c(), self.params.to_c()
        h = C.c_void_p()
        self._check(self._lib.mxs_dsa_create(C.byref(cg), C.byref(cp), VARIANTS[variant], float(probability),
                                             1 if p_mode == "arity" else 0, int(seed) & (2 ** 64 - 1),
                                             int(device), C.byref(h)))
        self._h = h
        # cost ties of a variable without neighbours break on the domain VALUE (relations.py:1661-1665):
        # only needed when some domain is not written in ascending order
        self._vrank = graph.value_rank()
        if self._vrank is not None:
            self._call("set_value_rank", self._vrank.ctypes.data)

    def reset(self):
        self._call("reset")

    def run(self, n_cycles: int):
        self._call("run", int(n_cycles))

    def assignment(self) -> Tuple[np.ndarray, np.ndarray]:
        idx = np.empty(self.graph.n_vars, dtype=np.int32)
        cost = np.empty(self.graph.n_vars)
        self._call("get_state", idx.ctypes.data, cost.ctypes.data)
        return idx, cost
