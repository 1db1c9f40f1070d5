"""DBA (pydcop/algorithms/dba.py) on the GPU: the ctypes binding of the `mxs_dba_*` entry points
(include/maxsum_gpu.h; device code: pydcop_amd/csrc/dba.h) on the same FlatGraph as the other
engines -- factors are the constraints, variables the DBA computations.  No CPU fallback."""
import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from ._binding import ReplicaBinding
from .engine import DBA_REPLICA_SYMBOLS as REPLICA_SYMBOLS, load_library
from .graph import FlatGraph, Params
from .mgm import name_ranks

INFINITY = 10000            # the reference's defaults (dba.py:265-268)
MAX_DISTANCE = 50
STOP_POLICIES = ("each", "first")


class DbaEngine(ReplicaBinding):
    """>>> eng = DbaEngine(graph, Params(mode="min"), infinity=1000, max_distance=50, seed=0)
    >>> eng.run(30)                                    # up to 30 rounds of (ok, improve)
    >>> eng.finished, eng.stop_round                   # a termination counter reached max_distance
    >>> idx, cost = eng.assignment()

    A table entry >= `infinity` is a violated constraint; nothing else of the tables is looked at.
    `mask_budget`: the most bytes the violation bits may take on the device (0: the library's default);
    an instance past it is refused before anything is allocated.

    `replicas=R`: R seeded runs of the instance in one engine (seeds `seed + r` modulo 2**64, or `seeds`), advanced
    by the two launches of one round over one copy of the violation bits; replica r is bit for bit the engine with
    that seed for as long as it runs.  `stop="each"`: a replica that stops is frozen, the engine has ended once all
    have stopped; `stop="first"`: the engine ends with the round in which the first replica stops.  A stop does not
    imply a solution, so the replicas are ranked by the constraints they still violate, counted on the device:
    >>> eng = DbaEngine(graph, infinity=1000, max_distance=5, replicas=8, seed=5, stop="each")
    >>> eng.run(60)
    >>> eng.stop_rounds, eng.violations()
    >>> eng.best()                                     # fewest violations, then earliest stop, then lowest index
    `replicas=1` without `seeds` and with `stop="each"` is the single run (`mxs_dba_create`: the same engine with
    one replica, launched through the single-run kernels)."""
    PREFIX = "mxs_dba"
    COUNTER = "rounds"
    STATE_FIELDS = (("idx", np.int32), ("cost", np.int32), ("has_cost", np.uint8), ("eval", np.int32),
                    ("improve", np.int32), ("new", np.int32), ("counter", np.int32), ("consistent", np.uint8))
    REPLICA_SYMBOLS = REPLICA_SYMBOLS
    REPLICA_FEATURE = "DBA's replicas"

    def __init__(self, graph: FlatGraph, params: Optional[Params] = None, infinity: float = INFINITY,
                 max_distance: int = MAX_DISTANCE, seed: int = 0, mask_budget: int = 0, device: int = 0,
                 lib_path: Optional[str] = None, replicas: int = 1, seeds: Optional[Sequence[int]] = None,
                 stop: str = "each"):
        if stop not in STOP_POLICIES:
            raise ValueError(f"Invalid value for parameter stop: {stop!r} (one of {list(STOP_POLICIES)})")
        self.infinity, self.max_distance, self.seed, self.stop = infinity, int(max_distance), int(seed), stop
        single = seeds is None and int(replicas) == 1 and stop == "each"
        sd = self._set_seeds(seed, seeds, replicas)     # (no seeds at all: the library refuses 0 replicas)
        self._lib = load_library(lib_path)
        self.graph = graph
        self.params = params or Params()
        cg, cp = graph.to_c(), self.params.to_c()
        self._rank = name_ranks(graph.var_names) if graph.var_names else None
        rank = None if self._rank is None else self._rank.ctypes.data
        h = C.c_void_p()
        if single:
            self._check(self._lib.mxs_dba_create(C.byref(cg), C.byref(cp), rank, float(infinity), self.max_distance,
                                                 self.seed & (2 ** 64 - 1), int(mask_budget), int(device), C.byref(h)))
        else:
            self._need_replica_symbols("replicas / seeds / stop need them")
            self._check(self._lib.mxs_dba_create_replicas(C.byref(cg), C.byref(cp), rank, float(infinity),
                                                          self.max_distance, sd.ctypes.data, self.replicas,
                                                          STOP_POLICIES.index(stop), int(mask_budget), int(device),
                                                          C.byref(h)))
        self._h = h

    def reset(self):
        self._call("reset")

    def run(self, n_rounds: int):
        """`n_rounds` more rounds, or as many as it takes to end; after the end, nothing."""
        self._call("run", int(n_rounds))

    def state(self, replica: int = 0) -> dict:
        """idx, cost (held; has_cost 0: still None), eval, improve, new (-1: still None), counter, consistent"""
        return super().state(replica)

    def assignment(self, replica: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        s = self.state(replica)
        return s["idx"], s["cost"].astype(np.float64)

    def weights(self, replica: int = 0) -> np.ndarray:
        """The weight of every slot = var_rowptr[v] + k (variable v, its k-th constraint) of `replica`."""
        out = np.empty(len(self.graph.var_edges), dtype=np.int32)
        if int(replica) == 0:       # (the call every version of the library has)
            self._call("get_weights", out.ctypes.data)
        else:
            self._need_replica_symbols("weights(replica) needs them")
            self._call("get_weights_replica", int(replica), out.ctypes.data)
        return out

    def _finished(self):
        stopped, at = C.c_int32(0), C.c_int64(0)
        self._call("finished", C.byref(stopped), C.byref(at))
        return bool(stopped.value), int(at.value)

    @property
    def finished(self) -> bool:
        """The engine has ended: every replica has stopped (`stop="each"`), or the first one has (`"first"`)."""
        return self._finished()[0]

    @property
    def stop_round(self) -> int:
        """The round in which the engine ended (0: not yet); a single run's: the round its stop condition held in."""
        return self._finished()[1]

    def _stop_rounds(self):
        self._need_replica_symbols("stop_rounds / rounds_of need them")
        stop = np.zeros(self.replicas, dtype=np.int64)
        ran = np.zeros(self.replicas, dtype=np.int64)
        self._call("stop_rounds", stop.ctypes.data, ran.ctypes.data)
        return stop, ran

    @property
    def stop_rounds(self) -> list:
        """Per replica, the round in which it stopped (0: it has not)."""
        return [int(x) for x in self._stop_rounds()[0]]

    @property
    def rounds_of(self) -> list:
        """Per replica, the rounds it ran."""
        return [int(x) for x in self._stop_rounds()[1]]

    def violations(self) -> np.ndarray:
        """Per replica, the constraints whose entry under its current assignment is >= `infinity`, counted on the
        device from the violation bits."""
        self._need_replica_symbols("violations needs them")
        out = np.zeros(self.replicas, dtype=np.int64)
        self._call("replica_violations", out.ctypes.data)
        return out

    def best(self) -> Dict:
        """The best replica's current state -- fewest violations, then earliest stop (running: last), then lowest
        index: {"replica", "stop_round", "violations", "idx"}."""
        self._need_replica_symbols("best needs them")
        r, stop, viol = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        self._call("best_replica", C.byref(r), C.byref(stop), C.byref(viol))
        return {"replica": int(r.value), "stop_round": int(stop.value), "violations": int(viol.value),
                "idx": self.state(int(r.value))["idx"]}

    @property
    def mask_bytes(self) -> int:
        n = C.c_int64(0)
        self._call("mask_bytes", C.byref(n))
        return int(n.value)
