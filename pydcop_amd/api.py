"""Direct API: solve a pyDCOP `DCOP` object (or a YAML file, or an .npz instance) on the GPU
without agents -- synchronous Max-Sum by default, `algo=` "amaxsum", "dsa", "mgm", "mgm2", "gdba" or "dba" for the other
engines of the library.

`pydcop.infrastructure.run.solve` (pydcop/infrastructure/run.py:49) deploys one
computation per node on agent threads and lets an orchestrator collect the values;
with `maxsum_gpu` those computations are proxies and the work is one engine anyway
(pydcop_amd/algorithms/maxsum_gpu.py).  This entry point goes straight from the DCOP
to the engine -- O(E) graph build, flat arrays, T cycles, values back -- and reports
with the reference's own `DCOP.solution_cost` (pydcop/dcop/dcop.py:308-367).
pyDCOP must be importable; nothing of it is modified.
"""
from importlib import import_module
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from .compile import assignment_to_values, compile_nodes
from .graph import FlatGraph, Params


class _Algo(NamedTuple):
    """What the front end knows of one algorithm.  `o` below: the keyword options of solve_dcop / solve_flat, by name."""
    engine: str = ""                                   # "module:class" in this package, imported when it is used
    engine_kw: Callable = lambda o: {}                 # o -> the keyword arguments of the engine's constructor
    seeded: bool = True                                # `seed` keys its draws (Max-Sum's only seeds the noise)
    noisy: bool = False                                # takes solve_dcop's `noise`
    restarts: Callable = lambda o: False               # o -> may `restarts` differ from 1
    best_every: bool = False                           # takes `best_every`
    draws: bool = False                                # takes `draws` other than "fixed"
    start: Callable = lambda eng, o: 0                 # before the run -> the period the engine traces by itself, or 0
    best: Callable = lambda eng, o: None               # after it -> (idx, the result's extra keys) in place of the
    #                                                    engine's assignment, or None
    end: Callable = lambda eng: {}                     # -> the extra keys of every result
    from_start: bool = False                           # run(n) counts from the start, not from where the engine is


def _many(o):
    return int(o["restarts"]) != 1


def _dsa_kw(o):
    return dict(variant=o["variant"], probability=o["probability"], p_mode=o["p_mode"], seed=o["seed"],
                replicas=int(o["restarts"]))


def _mgm_kw(o):
    return dict(draws=o["draws"], seed=o["seed"], replicas=int(o["restarts"])) if o["draws"] != "fixed" else {}


def _mgm2_kw(o):
    kw = dict(threshold=o["threshold"], favor=o["favor"], seed=o["seed"])
    return dict(kw, replicas=int(o["restarts"])) if _many(o) else kw          # (one run: mxs_mgm2_create, as ever)


def _gdba_kw(o):
    kw = dict(modifier=o["modifier"], violation=o["violation"], increase_mode=o["increase_mode"], seed=o["seed"])
    if _many(o) or int(o["best_every"]) != 0:                                 # (else one run: mxs_gdba_create, as ever)
        kw.update(seeds=[int(o["seed"]) + r for r in range(int(o["restarts"]))])
    return kw


def _dba_kw(o):
    kw = dict(infinity=o["dba_infinity"], max_distance=o["max_distance"], seed=o["seed"])
    # (one run: mxs_dba_create, as ever -- the two stop policies are the same thing there)
    return dict(kw, replicas=int(o["restarts"]), stop=o["dba_stop"]) if _many(o) else kw


def _track_records(eng, o):
    """algo="dsa" or "gdba" with best_every: every replica keeps its best state"""
    if int(o["best_every"]) > 0:
        eng.track_best(int(o["best_every"]), o["infinity"])
    return 0


def _best_record(eng, o):
    """algo="dsa" or "gdba" with restarts / best_every: (idx of the best replica -- its record when tracking, else its
    final state --, the result's extra keys); the device cost only ranks.  Else None."""
    if not _many(o) and int(o["best_every"]) == 0:
        return None
    if int(o["best_every"]) == 0:
        eng.track_best(0, o["infinity"])         # (no records: ranks the final states)
    best = eng.best()
    costs, _ = eng.replica_costs(o["infinity"])
    return best["idx"], {"replica": best["replica"], "best_cycle": best["cycle"],
                         "replica_costs": [float(c) for c in costs]}


def _best_final(eng, o):
    """algo="mgm" (keyed draws) or "mgm2" with restarts: (idx of the best replica's final state, the result's extra
    keys); the device cost only ranks.  Else None."""
    if not _many(o):
        return None
    best = eng.best(o["infinity"])
    costs, _ = eng.replica_costs(o["infinity"])
    return best["idx"], {"replica": best["replica"], "replica_costs": [float(c) for c in costs]}


def _dba_best(eng, o):
    """algo="dba" with restarts: (idx of the best replica's state -- fewest violated constraints, then earliest stop,
    ranked from the device's counts --, the result's extra keys).  Else None."""
    if not _many(o):
        return None
    best = eng.best()
    return best["idx"], {"replica": best["replica"], "replica_violations": [int(v) for v in eng.violations()],
                         "stop_rounds": eng.stop_rounds}


def _dba_end(eng):
    """DBA stops by itself: the rounds it ran and whether a termination counter reached max_distance"""
    return {"cycle": eng.cycle_count, "finished": eng.finished}


def _maxsum_track(eng, o):
    """algo="maxsum" with cost_every / best_every: switch the engine's device-side tracking on (one evaluation period
    for both: the record and the curve come from the same evaluations).  -> the period, 0 when there is none."""
    every = int(o["best_every"]) or int(o["cost_every"])
    if every <= 0 or (o["devices"] and int(o["devices"]) > 1):      # (the sharded engine keeps the host loop of _run_and_trace)
        return 0
    eng.track_best(every, o["infinity"], trace=int(o["cycles"]) // every + 2)
    return every


# the one description of every algorithm of `solve_dcop` / `solve_flat`; ALGOS is its order
_ALGOS = {
    "maxsum": _Algo("engine:MaxSumEngine", seeded=False, noisy=True, best_every=True, start=_maxsum_track),
    "amaxsum": _Algo("amaxsum:AMaxSumEngine", seeded=False, noisy=True, from_start=True),
    "dsa": _Algo("dsa:DsaEngine", _dsa_kw, restarts=lambda o: True, best_every=True, start=_track_records,
                 best=_best_record),
    "mgm": _Algo("mgm:MgmEngine", _mgm_kw, restarts=lambda o: o["draws"] == "keyed", draws=True, best=_best_final),
    "mgm2": _Algo("mgm2:Mgm2Engine", _mgm2_kw, restarts=lambda o: True, best=_best_final),
    # (a GDBA run's final state is usually not its best: restarts without records would rank wandering states)
    "gdba": _Algo("gdba:GdbaEngine", _gdba_kw, restarts=lambda o: int(o["best_every"]) >= 1, best_every=True,
                  start=_track_records, best=_best_record),
    "dba": _Algo("dba:DbaEngine", _dba_kw, restarts=lambda o: True, best=_dba_best, end=_dba_end),
}
_NO_ALGO = _Algo(seeded=False)             # (an unknown name takes no option; _engine_for refuses it)
ALGOS = tuple(_ALGOS)                      # the iterative ones: `cycles` of them
CLI_ALGOS = ALGOS + ("dpop",)              # DPOP has no cycles: solve_dcop_dpop / solve_flat_dpop

# `-p name:value` of the command line: the options of solve_flat / solve_yaml by name (`infinity`: dba_infinity)
CLI_PARAMS = {"damping": float, "stability": float, "noise": float, "seed": int,
              "damping_nodes": str, "start_messages": str, "precision": str, "devices": int,
              "variant": str, "probability": float, "p_mode": str, "threshold": float, "favor": str,
              "modifier": str, "violation": str, "increase_mode": str, "infinity": int, "max_distance": int,
              "restarts": int, "best_every": int, "draws": str, "dba_stop": str}


def _engine_for(graph: FlatGraph, params: Params, o: dict):
    """One engine on o["device"], or -- Max-Sum with devices > 1 -- the graph partitioned over GPUs
    0..devices-1 of this node (pydcop_amd.sharded.LocalShardedMaxSum: same surface, same result).
    Every engine has run / assignment / eval_cost / close."""
    algo, devices = o["algo"], o["devices"]
    if algo not in _ALGOS:
        raise ValueError(f"algo must be one of {ALGOS}" + (
            " (DPOP runs no cycles: solve_dcop_dpop / solve_flat_dpop)" if algo == "dpop" else ""))
    if devices and int(devices) > 1:
        if algo != "maxsum":
            raise ValueError("devices > 1: synchronous Max-Sum only")
        from .sharded import LocalShardedMaxSum
        return LocalShardedMaxSum(graph, params, list(range(int(devices))), lib_path=o["lib_path"])
    module, name = _ALGOS[algo].engine.split(":")
    engine = getattr(import_module("." + module, __package__), name)
    return engine(graph, params, device=o["device"], lib_path=o["lib_path"], **_ALGOS[algo].engine_kw(o))


def _run_and_trace(eng, from_start: bool, cycles: int, cost_every: int, infinity: float):
    """`cycles` cycles (amaxsum: generations of messages, its run() counts from the start), the
    cost evaluated on the device every `cost_every` of them."""
    curve: List[Tuple[int, float, int]] = []
    done = 0
    while done < cycles:
        n = min(cost_every, cycles - done) if cost_every > 0 else cycles - done
        eng.run(done + n if from_start else n)
        done += n
        if cost_every > 0:
            c, v = eng.eval_cost(infinity=infinity)
            curve.append((done, c, v))
    return curve


def _check_restarts(o):
    A, restarts, best_every, draws = _ALGOS.get(o["algo"], _NO_ALGO), o["restarts"], o["best_every"], o["draws"]
    if int(restarts) < 1 or int(best_every) < 0:
        raise ValueError("restarts must be at least 1 and best_every at least 0")
    if draws not in ("fixed", "keyed"):
        raise ValueError("draws must be \"fixed\" or \"keyed\"")
    if draws != "fixed" and not A.draws:
        raise ValueError("draws: algo=\"mgm\" only (the other local searches always key their draws on `seed`)")
    if int(restarts) != 1 and not A.restarts(o):
        raise ValueError("restarts: algo=\"dsa\", \"mgm2\" or \"dba\", algo=\"mgm\" with draws=\"keyed\", or algo=\"gdba\" "
                         "with best_every >= 1")
    if o["dba_stop"] not in ("first", "each"):
        raise ValueError("dba_stop must be \"first\" or \"each\"")
    if not A.best_every and int(best_every) != 0:
        raise ValueError("best_every: algo=\"dsa\", \"gdba\" or \"maxsum\" only")


def _check_maxsum_tracking(o):
    """the refusals of algo="maxsum" with best_every, before an engine exists"""
    if o["algo"] != "maxsum" or int(o["best_every"]) <= 0:
        return
    if int(o["cost_every"]) > 0 and int(o["best_every"]) != int(o["cost_every"]):
        raise ValueError("maxsum: cost_every and best_every are one evaluation period: give one, or the same value")
    if o["devices"] and int(o["devices"]) > 1:
        raise ValueError("best_every: maxsum on one device only (a shard's cost is partial)")


def _check_until_quiescent(o):
    """the refusals of until_quiescent, before an engine exists"""
    if int(o["until_quiescent"]) < 0:
        raise ValueError("until_quiescent must be at least 0")
    if int(o["until_quiescent"]) == 0:
        return
    if o["algo"] != "maxsum":
        raise ValueError("until_quiescent: algo=\"maxsum\" only (amaxsum ends by itself, the others have no send rule)")
    if o["devices"] and int(o["devices"]) > 1:
        raise ValueError("until_quiescent: maxsum on one device only (a shard sees its own edges only)")


def _checked(**o):
    """-> o, the options of one solve by name, after every refusal that needs no engine"""
    _check_restarts(o)
    _check_maxsum_tracking(o)
    _check_until_quiescent(o)
    return o


def _run_until_quiescent(eng, cycles, until_quiescent):
    """algo="maxsum" with until_quiescent = W: watch on the device, run until a cycle is found to have sent nothing,
    `cycles` at the most.  -> (the cycles run, the result's extra keys)"""
    eng.watch_quiescence(int(until_quiescent))
    ran = eng.run_until_quiescent(int(cycles))["cycles_run"]
    q = eng.quiescence()
    return ran, {"quiescent": q["quiescent"], "quiescent_cycle": q["cycle"], "active_edges": q["active"]}


def _maxsum_result(eng, cycles, cost_every, best_every, infinity):
    """-> (the curve of the device trace without its cycle-0 entry, or []; (idx, extra keys) of the record, or None)"""
    cyc, cost, viol, _ = eng.cost_trace()
    curve = [(int(c), float(x), int(v)) for c, x, v in zip(cyc, cost, viol) if c > 0] if int(cost_every) > 0 else []
    if int(cost_every) > 0 and int(cycles) % int(cost_every):      # (the curve ends with the last cycle, as ever)
        curve.append((int(cycles),) + tuple(eng.eval_cost(infinity=infinity)))
    if int(best_every) <= 0:
        return curve, None
    best = eng.best()
    return curve, (best["idx"], {"best_cycle": best["cycle"]})


def _solve(graph: FlatGraph, params: Params, o: dict, device_cost: bool):
    """One run of o["algo"] on the compiled instance, `o` as _checked returns it.  -> (idx of the selected assignment,
    the cycles run, the cost curve, the result's extra keys, with `device_cost` the engine's (cost, violation) of idx)"""
    A, cycles, cost_every, infinity = _ALGOS.get(o["algo"], _NO_ALGO), o["cycles"], o["cost_every"], o["infinity"]
    with _engine_for(graph, params, o) as eng:
        tracked = A.start(eng, o)
        if int(o["until_quiescent"]) > 0:
            cycles, ended = _run_until_quiescent(eng, cycles, o["until_quiescent"])
            curve = []
        else:
            curve, ended = _run_and_trace(eng, A.from_start, cycles, 0 if tracked else cost_every, infinity), {}  # (tracked: ONE run call)
        idx, _ = eng.assignment()
        extra = {**A.end(eng), **ended}
        best = A.best(eng, o)
        if tracked:
            curve, best = _maxsum_result(eng, cycles, cost_every, o["best_every"], infinity)
        if best:
            idx, more = best
            extra.update(more)
        measured = None
        if device_cost:
            measured = eng.eval_cost(idx, infinity=infinity) if best else eng.eval_cost(infinity=infinity)
    return idx, cycles, curve, extra, measured


def _values(graph: FlatGraph, idx) -> Dict:
    """the assignment by variable name and domain value; an instance without names: v0, v1, ... and the indices"""
    if graph.var_names is not None and graph.domains is not None:
        return assignment_to_values(graph, idx)
    return {f"v{i}": int(x) for i, x in enumerate(idx)}


def compile_dcop(dcop, noise: float = 0.0, seed: int = 0) -> FlatGraph:
    """DCOP -> FlatGraph in the node / links order the reference's factor graph has
    (pydcop/computations_graph/factor_graph.py:245-296), built in O(E)."""
    from . import plugin
    plugin.install()
    from pydcop.computations_graph import factor_graph_fast
    cg = factor_graph_fast.build_computation_graph(dcop)
    var_nodes = [n for n in cg.nodes if n.type == "VariableComputation"]
    factor_nodes = [n for n in cg.nodes if n.type == "FactorComputation"]
    return compile_nodes(var_nodes, factor_nodes, noise=noise, rng=np.random.default_rng(seed))


def solve_dcop(dcop, cycles: int = 30, *, damping: float = 0.5, damping_nodes: str = "both",
               stability: float = 0.1, noise: float = 0.01, start_messages: str = "leafs",
               precision: str = "f64", seed: int = 0, infinity: float = 10000, device: int = 0,
               cost_every: int = 0, lib_path: Optional[str] = None, devices: int = 1, algo: str = "maxsum",
               variant: str = "B", probability: float = 0.7, p_mode: str = "fixed", threshold: float = 0.5,
               favor: str = "unilateral", modifier: str = "A", violation: str = "NZ", increase_mode: str = "E",
               dba_infinity: int = 10000, max_distance: int = 50, restarts: int = 1, best_every: int = 0,
               draws: str = "fixed", dba_stop: str = "first", until_quiescent: int = 0) -> Dict:
    """Synchronous Max-Sum for exactly `cycles` cycles; parameters and defaults are those
    of `pydcop.algorithms.maxsum` (maxsum.py:212-220), `infinity` that of
    `pydcop.infrastructure.run.solve` (run.py:49).  `algo`: "amaxsum" (`cycles` = generations of
    messages under FIFO delivery, same parameters), "dsa" (`variant`, `probability`, `p_mode` of
    pydcop.algorithms.dsa, dsa.py:119-125; `seed` keys its draws), "mgm" or "mgm2" (`threshold`,
    `favor` of pydcop.algorithms.mgm2, mgm2.py:142-146; `seed` keys its draws) or "gdba" (`modifier`,
    `violation`, `increase_mode` of pydcop.algorithms.gdba, gdba.py:181-185; `seed` keys its draws) or "dba"
    (`dba_infinity`, `max_distance`: the `infinity` and `max_distance` of pydcop.algorithms.dba, dba.py:265-268 -- a
    cost >= dba_infinity is a violated constraint; min only; the run stops by itself, "cycle" is then the round it
    stopped in and "finished" is true; `seed` keys its draws); the local-search
    algorithms take no noise (their variable costs enter as the reference's do).

    algo="maxsum": Max-Sum on a loopy graph is not monotone, its last assignment is usually not its best.
    `best_every` = k > 0 keeps the best assignment seen at cycle 0 and after every k-th cycle on the device
    (MaxSumEngine.track_best: fewest violations, then cost): the assignment, cost and violation are then the record's
    and the result gains "best_cycle".  `cost_every` fills `cost_curve` from the same device trace, in one run call;
    alone it still reports the final state.  Both given and different: ValueError.  One device only.
    `until_quiescent` = W > 0 makes `cycles` a cap: the engine counts, on the device, the directed edges whose send
    counter is not at rest after every cycle c with c % W == 0 or c % W == 1 (MaxSumEngine.watch_quiescence) and the
    run ends once a cycle is found to have sent nothing -- every later cycle would repeat it.  "cycle" is then the
    number of cycles run and the result gains "quiescent", "quiescent_cycle" (None when the cap came first) and
    "active_edges" (the count of the last check); with `best_every` / `cost_every` the curve ends where the run ends.
    Any other algorithm, or `devices` > 1: ValueError.

    Returns {"assignment", "cost", "violation", "cycle", "cost_curve"}: the first three
    as `DCOP.solution_cost` computes them for the selected values; `cost_curve` (when
    `cost_every` > 0) = [(cycle, cost, violations)] evaluated on the device every
    `cost_every` cycles (the reference's `--collect_on cycle_change`,
    pydcop/commands/solve.py:356-376, without leaving the GPU).

    algo="dsa" only: `restarts` = R seeded runs (seeds seed .. seed + R - 1) in one engine, `best_every` = k > 0
    keeps every run's best state seen at cycle 0 and after every k-th cycle, on the device.  The assignment is then
    the best run's (its best record when tracking, else its final state; fewest violations, then cost, ranked on
    the device -- `cost` and `violation` are still `DCOP.solution_cost` of it) and the result gains "replica",
    "best_cycle" and "replica_costs" (the final states' device costs; `cost_curve` follows replica 0).

    algo="mgm": `draws` = "fixed" (the default: first domain value at start, first of equally good values) or "keyed"
    (both draws from the generator DSA uses, keyed on `seed`).  With draws="keyed", `restarts` = R seeded runs (seeds
    seed .. seed + R - 1) in one engine: the assignment is the best run's final state (fewest violations, then cost,
    ranked on the device) and the result gains "replica" and "replica_costs".  `best_every` stays DSA's: the sum MGM
    descends on never rises, so a run's final state is already its best and there is nothing to track.

    algo="mgm2": `restarts` = R seeded runs (seeds seed .. seed + R - 1) in one engine, the same way: the assignment is
    the best run's final state and the result gains "replica" and "replica_costs".

    algo="gdba": `best_every` = k > 0 and `restarts` as for DSA, rounds in place of cycles: the assignment is the best
    record of the best run and the result gains "replica", "best_cycle" and "replica_costs".  A GDBA run is not
    monotone (the breakout makes the assignment wander, its final state is usually not its best), so `restarts` > 1
    requires `best_every` >= 1.

    algo="dba": `restarts` = R seeded runs (seeds seed .. seed + R - 1) in one engine.  DBA's outcome depends entirely
    on its start draw and tie draws, and a stop does not imply a solution, so the assignment is that of the run with
    the fewest violated constraints (entries >= dba_infinity, counted on the device; then the earliest stop, then the
    lowest index).  `dba_stop` = "first" (the default): the engine ends with the round in which the first run stops,
    every run having completed it; "each": a run that stops is frozen, the others run on for `cycles` rounds or until
    all have stopped.  The result gains "replica", "replica_violations" and "stop_rounds" (0: that run has not
    stopped); "cycle" is the rounds the engine ran, "finished" whether it has ended.  `best_every` stays refused."""
    o = _checked(algo=algo, cycles=cycles, infinity=infinity, device=device, devices=devices, lib_path=lib_path,
                 cost_every=cost_every, until_quiescent=until_quiescent, variant=variant, probability=probability,
                 p_mode=p_mode, seed=seed, threshold=threshold, favor=favor, modifier=modifier, violation=violation,
                 increase_mode=increase_mode, dba_infinity=dba_infinity, max_distance=max_distance, restarts=restarts,
                 best_every=best_every, draws=draws, dba_stop=dba_stop)
    graph = compile_dcop(dcop, noise=noise if _ALGOS.get(algo, _NO_ALGO).noisy else 0.0, seed=seed)
    params = Params(mode=dcop.objective, damping=damping, damping_nodes=damping_nodes,
                    stability=stability, start_messages=start_messages, dtype=precision)
    idx, cycles, curve, extra, _ = _solve(graph, params, o, device_cost=False)
    assignment = assignment_to_values(graph, idx)
    violation, cost = dcop.solution_cost(assignment, infinity)
    return {"assignment": assignment, "cost": cost, "violation": violation, "cycle": cycles,
            "cost_curve": curve, **extra}


def solve_flat(graph: FlatGraph, objective: str = "min", cycles: int = 30, *, damping: float = 0.5,
               damping_nodes: str = "both", stability: float = 0.1, start_messages: str = "leafs",
               precision: str = "f64", infinity: float = 10000, device: int = 0, cost_every: int = 0,
               lib_path: Optional[str] = None, devices: int = 1, algo: str = "maxsum", variant: str = "B",
               probability: float = 0.7, p_mode: str = "fixed", seed: int = 0, threshold: float = 0.5,
               favor: str = "unilateral", modifier: str = "A", violation: str = "NZ", increase_mode: str = "E",
               dba_infinity: int = 10000, max_distance: int = 50, restarts: int = 1, best_every: int = 0,
               draws: str = "fixed", dba_stop: str = "first", until_quiescent: int = 0) -> Dict:
    """`solve_dcop` for an already compiled instance (`FlatGraph`, e.g. loaded from the
    .npz instance format): no pyDCOP import at all.  Cost and violations come from the
    device (`mxs_eval_cost` = DCOP.solution_cost, pydcop/dcop/dcop.py:308-367); noise, if
    wanted, is already folded into `graph.var_cost` by whoever compiled the instance."""
    params = Params(mode=objective, damping=damping, damping_nodes=damping_nodes,
                    stability=stability, start_messages=start_messages, dtype=precision)
    o = _checked(algo=algo, cycles=cycles, infinity=infinity, device=device, devices=devices, lib_path=lib_path,
                 cost_every=cost_every, until_quiescent=until_quiescent, variant=variant, probability=probability,
                 p_mode=p_mode, seed=seed, threshold=threshold, favor=favor, modifier=modifier, violation=violation,
                 increase_mode=increase_mode, dba_infinity=dba_infinity, max_distance=max_distance, restarts=restarts,
                 best_every=best_every, draws=draws, dba_stop=dba_stop)
    idx, cycles, curve, extra, (cost, violation) = _solve(graph, params, o, device_cost=True)
    return {"assignment": _values(graph, idx), "cost": cost, "violation": violation, "cycle": cycles,
            "cost_curve": curve, **extra}


def _solve_dpop(graph: FlatGraph, params: Params, tree, max_bytes, device, lib_path, infinity=None):
    """UTIL and VALUE on `tree` (None: `build_pseudotree` over the instance's order).  -> (idx, with an `infinity` the
    engine's (cost, violation) of it)"""
    from .dpop import DpopEngine
    with DpopEngine(graph, params, tree=tree, max_bytes=max_bytes, device=device, lib_path=lib_path) as eng:
        eng.solve()
        idx, _ = eng.assignment()
        return idx, (None if infinity is None else eng.eval_cost(infinity=infinity))


def solve_dcop_dpop(dcop, *, precision: str = "f64", infinity: float = 10000, device: int = 0, max_bytes: int = 0,
                    lib_path: Optional[str] = None) -> Dict:
    """DPOP (pydcop/algorithms/dpop.py): the exact optimum, on the pseudo-tree the reference builds for the DCOP
    (pydcop_amd/computations_graph/pseudotree_fast.py) and compiled as the dpop_gpu plug-in compiles it -- the
    assignment `pydcop solve --algo dpop` returns.  Same result keys as `solve_dcop`; "cycle" is 0."""
    from . import plugin
    plugin.install()
    from pydcop.computations_graph import pseudotree_fast
    from pydcop_amd.algorithms.dpop_gpu import compile_pseudotree
    graph, tree = compile_pseudotree(pseudotree_fast.build_computation_graph(dcop).nodes)
    idx, _ = _solve_dpop(graph, Params(mode=dcop.objective, dtype=precision), tree, max_bytes, device, lib_path)
    assignment = assignment_to_values(graph, idx)
    violation, cost = dcop.solution_cost(assignment, infinity)
    return {"assignment": assignment, "cost": cost, "violation": violation, "cycle": 0, "cost_curve": []}


def solve_flat_dpop(graph: FlatGraph, objective: str = "min", *, precision: str = "f64", infinity: float = 10000,
                    device: int = 0, max_bytes: int = 0, lib_path: Optional[str] = None) -> Dict:
    """`solve_dcop_dpop` for a compiled instance: the tree is `build_pseudotree` over the instance's variable
    and factor order; cost and violations are evaluated by the engine."""
    idx, (cost, violation) = _solve_dpop(graph, Params(mode=objective, dtype=precision), None, max_bytes, device, lib_path,
                                         infinity)
    return {"assignment": _values(graph, idx), "cost": cost, "violation": violation, "cycle": 0, "cost_curve": []}


def solve_yaml(paths, cycles: int = 30, **kw) -> Dict:
    """`solve_dcop` on DCOP YAML file(s) (pydcop/dcop/yamldcop.py:96)."""
    from . import plugin
    plugin.install()
    from pydcop.dcop.yamldcop import load_dcop_from_file
    if isinstance(paths, str):
        paths = [paths]
    return solve_dcop(load_dcop_from_file(list(paths)), cycles, **kw)


def main(argv=None):
    """`python -m pydcop_amd.api [-c CYCLES] [-p name:value ...] dcop.yaml ... | instance.npz`
    -- solve without agents and print a result in the schema of `pydcop solve`
    (docs/tutorials/analysing_results.rst:31-48; no agent metrics: there are no agents).
    `--export out.npz` compiles the YAML DCOP to the binary instance format instead
    (`FlatGraph.save`); an .npz instance is solved without importing pyDCOP."""
    import argparse
    import json
    import os
    import time
    ap = argparse.ArgumentParser(prog="python -m pydcop_amd.api")
    ap.add_argument("dcop_files", nargs="+")
    ap.add_argument("-c", "--cycles", type=int, default=30)
    ap.add_argument("-a", "--algo", default="maxsum", choices=CLI_ALGOS)   # (dpop: -c is ignored, cycle 0)
    ap.add_argument("-p", "--algo_params", action="append", default=[],
                    help="name:value, e.g. damping:0.7 noise:0 precision:f32 (maxsum.py:212-220)")
    ap.add_argument("--infinity", type=float, default=float("inf"))   # pydcop/commands/solve.py:316-324
    ap.add_argument("--cost_every", type=int, default=0)
    ap.add_argument("--until_quiescent", type=int, default=0, metavar="W",
                    help="maxsum: -c is a cap; stop once a cycle sent nothing, checked on the device every W cycles")
    ap.add_argument("--export", metavar="OUT.npz", default=None,
                    help="compile the YAML DCOP (noise folded in) and write it as an instance file")
    args = ap.parse_args(argv)
    kw = {}
    for item in args.algo_params:
        name, _, value = item.partition(":")
        if name not in CLI_PARAMS:
            raise SystemExit(f"Error: unknown parameter {name!r} (one of {sorted(CLI_PARAMS)})")
        kw[name] = CLI_PARAMS[name](value)
    if "infinity" in kw:          # (`--infinity` is the one of DCOP.solution_cost; this one is dba.py:266)
        kw["dba_infinity"] = kw.pop("infinity")
    t0 = time.perf_counter()
    if args.export:
        from . import plugin
        plugin.install()
        from pydcop.dcop.yamldcop import load_dcop_from_file
        dcop = load_dcop_from_file(list(args.dcop_files))
        g = compile_dcop(dcop, noise=kw.get("noise", 0.01), seed=kw.get("seed", 0))
        g.save(args.export, objective=dcop.objective, source=[os.path.basename(f) for f in args.dcop_files])
        print(json.dumps({"exported": args.export, "n_vars": g.n_vars, "n_factors": g.n_factors,
                          "n_edges": g.n_edges, "objective": dcop.objective}))
        return
    if len(args.dcop_files) == 1 and args.dcop_files[0].endswith(".npz"):
        graph, header = FlatGraph.load(args.dcop_files[0])
        kw.pop("noise", None)  # folded into the instance when it was compiled
        if args.algo == "dpop":
            res = solve_flat_dpop(graph, header.get("objective", "min"), infinity=args.infinity,
                                  precision=kw.get("precision", "f64"))
        else:
            if not _ALGOS[args.algo].seeded:       # (Max-Sum's seed is the noise's)
                kw.pop("seed", None)
            res = solve_flat(graph, header.get("objective", "min"), args.cycles, infinity=args.infinity,
                             cost_every=args.cost_every, algo=args.algo, until_quiescent=args.until_quiescent, **kw)
    elif args.algo == "dpop":
        from . import plugin
        plugin.install()
        from pydcop.dcop.yamldcop import load_dcop_from_file
        res = solve_dcop_dpop(load_dcop_from_file(list(args.dcop_files)), infinity=args.infinity,
                              precision=kw.get("precision", "f64"))
    else:
        res = solve_yaml(args.dcop_files, args.cycles, infinity=args.infinity,
                         cost_every=args.cost_every, algo=args.algo, until_quiescent=args.until_quiescent, **kw)
    out = {"assignment": res["assignment"], "cost": res["cost"], "violation": res["violation"],
           "cycle": res["cycle"], "status": "FINISHED", "time": time.perf_counter() - t0,
           "msg_count": 0, "msg_size": 0, "agt_metrics": {}}
    if res["cost_curve"]:
        out["cost_curve"] = res["cost_curve"]
    for key in ("replica", "best_cycle", "replica_costs", "replica_violations", "stop_rounds",  # (-p restarts / best_every)
                "quiescent", "quiescent_cycle", "active_edges"):                                # (--until_quiescent)
        if key in res:
            out[key] = res[key]
    print(json.dumps(out, sort_keys=True, indent="  "))


if __name__ == "__main__":
    main()
