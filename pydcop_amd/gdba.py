"""GDBA (pydcop/algorithms/gdba.py) on the GPU: the ctypes binding of the `mxs_gdba_*` entry points
(include/maxsum_gpu.h; device code: pydcop_amd/csrc/gdba.h) on the same FlatGraph as the other
engines -- factors are the constraints, variables the GDBA computations.  No CPU fallback."""
import ctypes as C
from typing import Optional, Tuple

import numpy as np

from ._binding import EngineBinding
from .engine import load_library
from .graph import FlatGraph, Params
from .mgm import name_ranks

MODIFIERS = ("A", "M")
VIOLATIONS = ("NZ", "NM", "MX")
INCREASE_MODES = ("E", "R", "C", "T")
MAX_ROUNDS = 65535          # the modifier counters are 16 bits wide (mxs_gdba_run refuses to go past it)


def check_params(modifier, violation, increase_mode):
    """The reference's parameter definitions (gdba.py:181-185)."""
    for name, value, choices in (("modifier", modifier, MODIFIERS), ("violation", violation, VIOLATIONS),
                                 ("increase_mode", increase_mode, INCREASE_MODES)):
        if value not in choices:
            raise ValueError(f"Invalid value for parameter {name}: {value!r} (one of {list(choices)})")
    return MODIFIERS.index(modifier), VIOLATIONS.index(violation), INCREASE_MODES.index(increase_mode)


class GdbaEngine(EngineBinding):
    """>>> eng = GdbaEngine(graph, Params(mode="min"), modifier="A", violation="NZ", increase_mode="E", seed=0)
    >>> eng.run(30)                                    # 30 rounds of (ok, improve)
    >>> idx, cost = eng.assignment()

    `pool_budget`: the most bytes the modifier tables may take on the device (0: the library's default);
    an instance past it is refused before anything is allocated."""
    PREFIX = "mxs_gdba"
    COUNTER = "rounds"

    def __init__(self, graph: FlatGraph, params: Optional[Params] = None, modifier: str = "A", violation: str = "NZ",
                 increase_mode: str = "E", seed: int = 0, pool_budget: int = 0, device: int = 0,
                 lib_path: Optional[str] = None):
        codes = check_params(modifier, violation, increase_mode)
        self.modifier, self.violation, self.increase_mode, self.seed = modifier, violation, increase_mode, int(seed)
        self._lib = load_library(lib_path)
        self.graph = graph
        self.params = params or Params()
        cg, cp = graph.to_c(), self.params.to_c()
        self._rank = name_ranks(graph.var_names) if graph.var_names else None
        # cost ties of a variable without neighbours break on the domain VALUE (relations.py:1661-1665)
        self._vrank = graph.value_rank()
        h = C.c_void_p()
        self._check(self._lib.mxs_gdba_create(C.byref(cg), C.byref(cp),
                                              None if self._rank is None else self._rank.ctypes.data,
                                              None if self._vrank is None else self._vrank.ctypes.data,
                                              codes[0], codes[1], codes[2], self.seed & (2 ** 64 - 1),
                                              int(pool_budget), int(device), C.byref(h)))
        self._h = h

    def reset(self):
        self._call("reset")

    def run(self, n_rounds: int):
        self._call("run", int(n_rounds))

    def state(self) -> dict:
        n = self.graph.n_vars
        out = {"idx": np.empty(n, dtype=np.int32), "cost": np.empty(n), "has_cost": np.empty(n, dtype=np.uint8),
               "improve": np.empty(n), "new": np.empty(n, dtype=np.int32)}
        self._call("get_state", *[out[k].ctypes.data for k in ("idx", "cost", "has_cost", "improve", "new")])
        return out

    def assignment(self) -> Tuple[np.ndarray, np.ndarray]:
        s = self.state()
        return s["idx"], s["cost"]

    def modifiers(self, slot: int) -> np.ndarray:
        """The modifier table of slot = var_rowptr[v] + k (variable v, its k-th constraint), in the layout of the
        constraint's table; one entry in mode T; empty where the engine stores none (no look-up can reach it)."""
        n = C.c_int64(0)
        self._call("get_modifiers", int(slot), None, 0, C.byref(n))
        out = np.empty(int(n.value), dtype=np.int32)
        if n.value:
            self._call("get_modifiers", int(slot), out.ctypes.data, int(n.value), C.byref(n))
        return out

    @property
    def pool_bytes(self) -> int:
        n = C.c_int64(0)
        self._call("get_modifiers", -1, None, 0, C.byref(n))
        return int(n.value)
