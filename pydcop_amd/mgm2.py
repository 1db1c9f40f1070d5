"""MGM-2 (pydcop/algorithms/mgm2.py) on the GPU: the ctypes binding of the `mxs_mgm2_*` entry points
(include/maxsum_gpu.h; device code: pydcop_amd/csrc/mgm2.h) on the same FlatGraph as the other
engines -- factors are the constraints, variables the MGM-2 computations.  No CPU fallback."""
import ctypes as C
from typing import Optional, Tuple

import numpy as np

from ._binding import EngineBinding
from .engine import load_library
from .graph import FlatGraph, Params
from .mgm import name_ranks

FAVORS = ("unilateral", "no", "coordinated")


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


class Mgm2Engine(EngineBinding):
    """>>> eng = Mgm2Engine(graph, Params(mode="min"), threshold=0.5, favor="unilateral", seed=0)
    >>> eng.run(30)                                    # 30 rounds (= the reference's stop_cycle 31)
    >>> idx, cost = eng.assignment()
    """
    PREFIX = "mxs_mgm2"
    COUNTER = "rounds"

    def __init__(self, graph: FlatGraph, params: Optional[Params] = None, threshold: float = 0.5,
                 favor: str = "unilateral", seed: int = 0, device: int = 0, lib_path: Optional[str] = None):
        self.threshold, favor_code = check_params(threshold, favor)
        self.favor, self.seed = favor, int(seed)
        self._lib = load_library(lib_path)
        self.graph = graph
        self.params = params or Params()
        cg, cp = graph.to_c(), self.params.to_c()
        self._rank = name_ranks(graph.var_names) if graph.var_names else None
        h = C.c_void_p()
        self._check(self._lib.mxs_mgm2_create(C.byref(cg), C.byref(cp),
                                              None if self._rank is None else self._rank.ctypes.data,
                                              self.threshold, favor_code, self.seed & (2 ** 64 - 1), int(device),
                                              C.byref(h)))
        self._h = h

    def reset(self):
        self._call("reset")

    def run(self, n_rounds: int):
        self._call("run", int(n_rounds))

    def state(self) -> dict:
        n = self.graph.n_vars
        out = {"idx": np.empty(n, dtype=np.int32), "cost": np.empty(n), "has_cost": np.empty(n, dtype=np.uint8)}
        self._call("get_state", *[out[k].ctypes.data for k in ("idx", "cost", "has_cost")])
        return out

    def assignment(self) -> Tuple[np.ndarray, np.ndarray]:
        s = self.state()
        return s["idx"], s["cost"]
