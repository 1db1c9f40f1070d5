"""What the ctypes bindings of the `mxs_dsa_*`, `mxs_mgm_*`, `mxs_mgm2_*`, `mxs_gdba_*`, `mxs_dba_*` and `mxs_dpop_*` entry points
(include/maxsum_gpu.h) share: the handle, the error check, `eval_cost`, the cycle counter and the life cycle."""
import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from .engine import MaxSumGpuError


class EngineBinding:
    """A class sets PREFIX (`mxs_gdba`) and COUNTER (`rounds`: the entry point `mxs_gdba_rounds`), loads
    `self._lib` and stores the handle of `<PREFIX>_create` in `self._h`."""
    PREFIX = ""
    COUNTER = ""
    _h = None

    def _check(self, rc: int):
        if rc != 0:
            raise MaxSumGpuError(f"maxsum_gpu error {rc}: {self._lib.mxs_last_error().decode()}")

    def _call(self, name: str, *args):
        """<PREFIX>_<name>(handle, *args), checked"""
        self._check(getattr(self._lib, f"{self.PREFIX}_{name}")(self._h, *args))

    @property
    def cycle_count(self) -> int:
        n = C.c_int64(0)
        self._call(self.COUNTER, C.byref(n))
        return int(n.value)

    def eval_cost(self, idx=None, infinity: float = float("inf")) -> Tuple[float, int]:
        cost, viol = C.c_double(0), C.c_int64(0)
        p = None
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            p = idx.ctypes.data
        self._call("eval_cost", p, float(infinity), C.byref(cost), C.byref(viol))
        return float(cost.value), int(viol.value)

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._lib, f"{self.PREFIX}_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class ReplicaBinding(EngineBinding):
    """What the bindings of the replica engines (`DsaEngine`, `MgmEngine`, `Mgm2Engine`, `GdbaEngine`: R seeded runs
    in one engine) share.  A class with `state()` sets STATE_FIELDS, the (key, dtype) pairs of `<PREFIX>_get_state`'s
    arrays in argument order; one whose replicas came after its first release sets REPLICA_SYMBOLS, the entry points
    they need, and REPLICA_FEATURE, what the message calls them."""
    STATE_FIELDS: Tuple[Tuple[str, type], ...] = ()
    REPLICA_SYMBOLS: Tuple[str, ...] = ()
    REPLICA_FEATURE = ""

    def _need_replica_symbols(self, why: str):
        missing = [n for n in self.REPLICA_SYMBOLS if not hasattr(self._lib, n)]
        if missing:
            raise MaxSumGpuError(
                f"{self._lib._name} was built from sources without {self.REPLICA_FEATURE} (no {', '.join(missing)}): "
                f"rebuild the library, {why}")

    def state(self, replica: int = 0) -> dict:
        n = self.graph.n_vars
        out = {key: np.empty(n, dtype=dtype) for key, dtype in self.STATE_FIELDS}
        ptrs = [a.ctypes.data for a in out.values()]
        if int(replica) == 0:       # (the call every version of the library has)
            self._call("get_state", *ptrs)
        else:
            self._need_replica_symbols("state(replica) needs them")
            self._call("get_state_replica", int(replica), *ptrs)
        return out

    def assignment(self, replica: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        s = self.state(replica)
        return s["idx"], s["cost"]

    def _set_seeds(self, seed: int, seeds: Optional[Sequence[int]], replicas: int) -> np.ndarray:
        """`self.seeds` (`seed + r` modulo 2**64, or `seeds`) and `self.replicas`; the array `<PREFIX>_create_*` takes"""
        if seeds is None:
            seeds = [int(seed) + r for r in range(int(replicas))]
        elif replicas not in (1, len(seeds)):
            raise ValueError(f"{len(seeds)} seeds for {replicas} replicas")
        self.seeds = [int(x) & (2 ** 64 - 1) for x in seeds]
        self.replicas = len(self.seeds)
        return np.array(self.seeds, dtype=np.uint64)

    def _set_value_rank(self):
        """cost ties of a variable without neighbours break on the domain VALUE (relations.py:1661-1665):
        only needed when some domain is not written in ascending order"""
        self._vrank = self.graph.value_rank()
        if self._vrank is not None:
            self._call("set_value_rank", self._vrank.ctypes.data)

    def replica_costs(self, infinity: float = float("inf")) -> Tuple[np.ndarray, np.ndarray]:
        """(cost[R], violations[R]) of the replicas' current assignments, reduced on the device: what
        `eval_cost(assignment(r)[0], infinity)` gives, in a fixed summation order of its own."""
        cost = np.empty(self.replicas)
        viol = np.empty(self.replicas, dtype=np.int64)
        self._call("replica_costs", float(infinity), cost.ctypes.data, viol.ctypes.data)
        return cost, viol

    # what the public `track_best` / `best` of the engines call after their own guard (the docstrings are theirs)

    def _track_best(self, every: int, infinity: float):
        self._call("track_best", int(every), float(infinity))

    def _best_record(self, replica: int) -> Dict:
        """`<PREFIX>_get_best`: the record of an engine that tracks the best state"""
        r, cyc, cost, viol = C.c_int32(0), C.c_int64(0), C.c_double(0), C.c_int64(0)
        idx = np.empty(self.graph.n_vars, dtype=np.int32)
        self._call("get_best", int(replica), C.byref(r), C.byref(cyc), C.byref(cost), C.byref(viol), idx.ctypes.data)
        return {"replica": int(r.value), "cycle": int(cyc.value), "cost": float(cost.value),
                "violations": int(viol.value), "idx": idx}

    def _best_ranked(self, infinity: float) -> Dict:
        """`<PREFIX>_best_replica`: the best current state of an engine that keeps no records"""
        r, cost, viol = C.c_int32(0), C.c_double(0), C.c_int64(0)
        self._call("best_replica", float(infinity), C.byref(r), C.byref(cost), C.byref(viol))
        return {"replica": int(r.value), "cost": float(cost.value), "violations": int(viol.value),
                "idx": self.state(int(r.value))["idx"]}
