"""GDBA (pydcop/algorithms/gdba.py) on the GPU: the ctypes binding of the `mxs_gdba_*` entry points
(include/maxsum_gpu.h; device code: pydcop_amd/csrc/gdba.h) on the same FlatGraph as the other
engines -- factors are the constraints, variables the GDBA computations.  No CPU fallback."""
import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from ._binding import ReplicaBinding
from .engine import GDBA_REPLICA_SYMBOLS as REPLICA_SYMBOLS, load_library
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


class GdbaEngine(ReplicaBinding):
    """>>> eng = GdbaEngine(graph, Params(mode="min"), modifier="A", violation="NZ", increase_mode="E", seed=0)
    >>> eng.run(30)                                    # 30 rounds of (ok, improve)
    >>> idx, cost = eng.assignment()

    `pool_budget`: the most bytes the modifier tables may take on the device (0: the library's default), those of
    all replicas together; an instance past it is refused before anything is allocated.

    `replicas=R`: R seeded runs of the instance in one engine (seeds `seed + r` modulo 2**64, or `seeds`), advanced
    by the two launches of one round over one copy of the tables; replica r is bit for bit the engine with that
    seed, its modifier tables included.  A GDBA run is not monotone -- the breakout makes the assignment wander --
    so keep every run's best state, on the device:
    >>> eng = GdbaEngine(graph, modifier="M", violation="NM", increase_mode="T", replicas=8, seed=5)
    >>> eng.track_best(every=1, infinity=10000)
    >>> eng.run(30)
    >>> eng.best()                                     # the best replica's record
    `replicas=1` without `seeds` is the single run (`mxs_gdba_create`: the same engine with one replica, launched
    through the single-run kernels); it tracks no best state."""
    PREFIX = "mxs_gdba"
    COUNTER = "rounds"
    STATE_FIELDS = (("idx", np.int32), ("cost", np.float64), ("has_cost", np.uint8), ("improve", np.float64),
                    ("new", np.int32))
    REPLICA_SYMBOLS = REPLICA_SYMBOLS
    REPLICA_FEATURE = "GDBA's replicas"

    def __init__(self, graph: FlatGraph, params: Optional[Params] = None, modifier: str = "A", violation: str = "NZ",
                 increase_mode: str = "E", seed: int = 0, pool_budget: int = 0, device: int = 0,
                 lib_path: Optional[str] = None, seeds: Optional[Sequence[int]] = None, replicas: int = 1):
        codes = check_params(modifier, violation, increase_mode)
        self.modifier, self.violation, self.increase_mode, self.seed = modifier, violation, increase_mode, int(seed)
        single = seeds is None and int(replicas) == 1
        sd = self._set_seeds(seed, seeds, replicas)     # (no seeds at all: the library refuses 0 replicas)
        self._lib = load_library(lib_path)
        self.graph = graph
        self.params = params or Params()
        cg, cp = graph.to_c(), self.params.to_c()
        self._rank = name_ranks(graph.var_names) if graph.var_names else None
        # cost ties of a variable without neighbours break on the domain VALUE (relations.py:1661-1665)
        self._vrank = graph.value_rank()
        rank = None if self._rank is None else self._rank.ctypes.data
        vrank = None if self._vrank is None else self._vrank.ctypes.data
        h = C.c_void_p()
        if single:
            self._check(self._lib.mxs_gdba_create(C.byref(cg), C.byref(cp), rank, vrank, codes[0], codes[1], codes[2],
                                                  self.seed & (2 ** 64 - 1), int(pool_budget), int(device), C.byref(h)))
        else:
            self._need_replica_symbols("replicas / seeds need them")
            self._check(self._lib.mxs_gdba_create_replicas(C.byref(cg), C.byref(cp), rank, vrank, codes[0], codes[1],
                                                           codes[2], sd.ctypes.data, self.replicas, int(pool_budget),
                                                           int(device), C.byref(h)))
        self._h = h

    def reset(self):
        self._call("reset")

    def run(self, n_rounds: int):
        self._call("run", int(n_rounds))

    def modifiers(self, slot: int, replica: int = 0) -> np.ndarray:
        """The modifier table of slot = var_rowptr[v] + k (variable v, its k-th constraint) of `replica`, in the layout
        of the constraint's table; one entry in mode T; empty where the engine stores none (no look-up can reach it)."""
        if int(replica) == 0:
            get = lambda *a: self._call("get_modifiers", *a)                                # noqa: E731
        else:
            self._need_replica_symbols("modifiers(slot, replica) needs them")
            get = lambda *a: self._call("get_modifiers_replica", int(replica), *a)          # noqa: E731
        n = C.c_int64(0)
        get(int(slot), None, 0, C.byref(n))
        out = np.empty(int(n.value), dtype=np.int32)
        if n.value:
            get(int(slot), out.ctypes.data, int(n.value), C.byref(n))
        return out

    @property
    def pool_bytes(self) -> int:
        """the bytes of the modifier tables, all replicas"""
        n = C.c_int64(0)
        self._call("get_modifiers", -1, None, 0, C.byref(n))
        return int(n.value)

    def replica_costs(self, infinity: float = float("inf")) -> Tuple[np.ndarray, np.ndarray]:
        self._need_replica_symbols("replica_costs needs them")
        return super().replica_costs(infinity)

    def track_best(self, every: int = 1, infinity: float = float("inf")):
        """Keep, per replica, the best state seen now and after every `every`-th round (0: off; the `infinity` then
        only serves `best()`).  Clears the records.  The replica engine's (`replicas` > 1, or `seeds`)."""
        self._need_replica_symbols("track_best needs them")
        self._track_best(every, infinity)

    def best(self, replica: int = -1) -> Dict:
        """The record of `replica` (-1: of the best replica: fewest violations, then best cost, then lowest
        index) when tracking is on, else its current state: {"replica", "cycle", "cost", "violations", "idx"},
        "cycle" the round of the record."""
        self._need_replica_symbols("best needs them")
        return self._best_record(replica)
