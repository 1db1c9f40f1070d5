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
from typing import Dict, List, Optional, Tuple

import numpy as np

from .compile import assignment_to_values, compile_nodes
from .graph import FlatGraph, Params


ALGOS = ("maxsum", "amaxsum", "dsa", "mgm", "mgm2", "gdba", "dba")    # the iterative ones: `cycles` of them
CLI_ALGOS = ALGOS + ("dpop",)                              # DPOP has no cycles: solve_dcop_dpop / solve_flat_dpop


def _engine_for(graph: FlatGraph, params: Params, device: int, devices: int, lib_path, algo: str = "maxsum",
                algo_kw: Optional[dict] = None):
    """One engine on `device`, or -- Max-Sum with devices > 1 -- the graph partitioned over GPUs
    0..devices-1 of this node (pydcop_amd.sharded.LocalShardedMaxSum: same surface, same result).
    Every engine has run / assignment / eval_cost / close."""
    algo_kw = algo_kw or {}
    if algo not in ALGOS:
        raise ValueError(f"algo must be one of {ALGOS}" + (
            " (DPOP runs no cycles: solve_dcop_dpop / solve_flat_dpop)" if algo == "dpop" else ""))
    if algo != "maxsum":
        if devices and int(devices) > 1:
            raise ValueError("devices > 1: synchronous Max-Sum only")
        if algo == "amaxsum":
            from .amaxsum import AMaxSumEngine
            return AMaxSumEngine(graph, params, device=device, lib_path=lib_path)
        if algo == "dsa":
            from .dsa import DsaEngine
            return DsaEngine(graph, params, device=device, lib_path=lib_path, **algo_kw)
        if algo == "mgm2":
            from .mgm2 import Mgm2Engine
            return Mgm2Engine(graph, params, device=device, lib_path=lib_path, **algo_kw)
        if algo == "gdba":
            from .gdba import GdbaEngine
            return GdbaEngine(graph, params, device=device, lib_path=lib_path, **algo_kw)
        if algo == "dba":
            from .dba import DbaEngine
            return DbaEngine(graph, params, device=device, lib_path=lib_path, **algo_kw)
        from .mgm import MgmEngine
        return MgmEngine(graph, params, device=device, lib_path=lib_path, **algo_kw)
    from .engine import MaxSumEngine
    if devices and int(devices) > 1:
        from .sharded import LocalShardedMaxSum
        return LocalShardedMaxSum(graph, params, list(range(int(devices))), lib_path=lib_path)
    return MaxSumEngine(graph, params, device=device, lib_path=lib_path)


def _algo_kw(algo, variant, probability, p_mode, seed, threshold, favor, modifier="A", violation="NZ",
             increase_mode="E", dba_infinity=10000, max_distance=50, restarts=1, draws="fixed", best_every=0,
             dba_stop="first"):
    if algo == "dba":
        kw = dict(infinity=dba_infinity, max_distance=max_distance, seed=seed)
        # (one run: mxs_dba_create, as ever -- the two stop policies are the same thing there)
        return dict(kw, replicas=int(restarts), stop=dba_stop) if int(restarts) != 1 else kw
    if algo == "gdba":
        kw = dict(modifier=modifier, violation=violation, increase_mode=increase_mode, seed=seed)
        if int(restarts) != 1 or int(best_every) != 0:      # (else one run: mxs_gdba_create, as ever)
            kw.update(seeds=[int(seed) + r for r in range(int(restarts))])
        return kw
    if algo == "dsa":
        return dict(variant=variant, probability=probability, p_mode=p_mode, seed=seed, replicas=int(restarts))
    if algo == "mgm2":
        kw = dict(threshold=threshold, favor=favor, seed=seed)
        return dict(kw, replicas=int(restarts)) if int(restarts) != 1 else kw     # (one run: mxs_mgm2_create, as ever)
    if algo == "mgm" and draws != "fixed":
        return dict(draws=draws, seed=seed, replicas=int(restarts))
    return None


def _run_and_trace(eng, algo: str, cycles: int, cost_every: int, infinity: float):
    """`cycles` cycles (amaxsum: generations of messages, its run() counts from the start), the
    cost evaluated on the device every `cost_every` of them."""
    curve: List[Tuple[int, float, int]] = []
    done = 0
    while done < cycles:
        n = min(cost_every, cycles - done) if cost_every > 0 else cycles - done
        eng.run(done + n if algo == "amaxsum" else n)
        done += n
        if cost_every > 0:
            c, v = eng.eval_cost(infinity=infinity)
            curve.append((done, c, v))
    return curve


def _check_restarts(algo, restarts, best_every, draws="fixed", dba_stop="first"):
    if int(restarts) < 1 or int(best_every) < 0:
        raise ValueError("restarts must be at least 1 and best_every at least 0")
    if draws not in ("fixed", "keyed"):
        raise ValueError("draws must be \"fixed\" or \"keyed\"")
    if draws != "fixed" and algo != "mgm":
        raise ValueError("draws: algo=\"mgm\" only (the other local searches always key their draws on `seed`)")
    # (a GDBA run's final state is usually not its best: restarts without records would rank wandering states)
    if int(restarts) != 1 and not (algo in ("dsa", "mgm2", "dba") or (algo == "mgm" and draws == "keyed")
                                   or (algo == "gdba" and int(best_every) >= 1)):
        raise ValueError("restarts: algo=\"dsa\", \"mgm2\" or \"dba\", algo=\"mgm\" with draws=\"keyed\", or algo=\"gdba\" "
                         "with best_every >= 1")
    if dba_stop not in ("first", "each"):
        raise ValueError("dba_stop must be \"first\" or \"each\"")
    if algo not in ("dsa", "gdba", "maxsum") and int(best_every) != 0:
        raise ValueError("best_every: algo=\"dsa\", \"gdba\" or \"maxsum\" only")


def _check_maxsum_tracking(algo, cost_every, best_every, devices):
    """the refusals of algo="maxsum" with best_every, before an engine exists"""
    if algo != "maxsum" or int(best_every) <= 0:
        return
    if int(cost_every) > 0 and int(best_every) != int(cost_every):
        raise ValueError("maxsum: cost_every and best_every are one evaluation period: give one, or the same value")
    if devices and int(devices) > 1:
        raise ValueError("best_every: maxsum on one device only (a shard's cost is partial)")


def _check_until_quiescent(algo, until_quiescent, devices):
    """the refusals of until_quiescent, before an engine exists"""
    if int(until_quiescent) < 0:
        raise ValueError("until_quiescent must be at least 0")
    if int(until_quiescent) == 0:
        return
    if algo != "maxsum":
        raise ValueError("until_quiescent: algo=\"maxsum\" only (amaxsum ends by itself, the others have no send rule)")
    if devices and int(devices) > 1:
        raise ValueError("until_quiescent: maxsum on one device only (a shard sees its own edges only)")


def _run_until_quiescent(eng, cycles, until_quiescent):
    """algo="maxsum" with until_quiescent = W: watch on the device, run until a cycle is found to have sent nothing,
    `cycles` at the most.  -> (the cycles run, the result's extra keys)"""
    eng.watch_quiescence(int(until_quiescent))
    ran = eng.run_until_quiescent(int(cycles))["cycles_run"]
    q = eng.quiescence()
    return ran, {"quiescent": q["quiescent"], "quiescent_cycle": q["cycle"], "active_edges": q["active"]}


def _maxsum_track(eng, algo, cycles, cost_every, best_every, infinity, devices=1):
    """algo="maxsum" with cost_every / best_every: switch the engine's device-side tracking on (one evaluation period
    for both: the record and the curve come from the same evaluations).  -> the period, 0 when there is none."""
    every = int(best_every) or int(cost_every)
    if algo != "maxsum" or every <= 0:
        return 0
    if devices and int(devices) > 1:
        return 0                     # (the sharded engine keeps the host loop of _run_and_trace)
    eng.track_best(every, infinity, trace=int(cycles) // every + 2)
    return every


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


def _dsa_best(eng, algo, restarts, best_every, infinity):
    """algo="dsa" or "gdba" with restarts / best_every: (idx of the best replica -- its record when tracking, else its
    final state --, the result's extra keys); the device cost only ranks.  Else None."""
    if algo not in ("dsa", "gdba") or (int(restarts) == 1 and int(best_every) == 0):
        return None
    if int(best_every) == 0:
        eng.track_best(0, infinity)         # (no records: ranks the final states)
    best = eng.best()
    costs, _ = eng.replica_costs(infinity)
    return best["idx"], {"replica": best["replica"], "best_cycle": best["cycle"],
                         "replica_costs": [float(c) for c in costs]}


def _mgm_best(eng, algo, restarts, infinity):
    """algo="mgm" (keyed draws) or "mgm2" with restarts: (idx of the best replica's final state, the result's extra
    keys); the device cost only ranks.  Else None."""
    if algo not in ("mgm", "mgm2") or int(restarts) == 1:
        return None
    best = eng.best(infinity)
    costs, _ = eng.replica_costs(infinity)
    return best["idx"], {"replica": best["replica"], "replica_costs": [float(c) for c in costs]}


def _dba_best(eng, algo, restarts):
    """algo="dba" with restarts: (idx of the best replica's state -- fewest violated constraints, then earliest stop,
    ranked from the device's counts --, the result's extra keys).  Else None."""
    if algo != "dba" or int(restarts) == 1:
        return None
    best = eng.best()
    return best["idx"], {"replica": best["replica"], "replica_violations": [int(v) for v in eng.violations()],
                         "stop_rounds": eng.stop_rounds}


def _dba_end(eng, algo):
    """DBA stops by itself: the rounds it ran and whether a termination counter reached max_distance"""
    return {"cycle": eng.cycle_count, "finished": eng.finished} if algo == "dba" else {}


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
    _check_restarts(algo, restarts, best_every, draws, dba_stop)
    _check_maxsum_tracking(algo, cost_every, best_every, devices)
    _check_until_quiescent(algo, until_quiescent, devices)
    graph = compile_dcop(dcop, noise=noise if algo in ("maxsum", "amaxsum") else 0.0, seed=seed)
    params = Params(mode=dcop.objective, damping=damping, damping_nodes=damping_nodes,
                    stability=stability, start_messages=start_messages, dtype=precision)
    algo_kw = _algo_kw(algo, variant, probability, p_mode, seed, threshold, favor, modifier, violation, increase_mode,
                       dba_infinity, max_distance, restarts, draws, best_every, dba_stop)
    with _engine_for(graph, params, device, devices, lib_path, algo, algo_kw) as eng:
        if algo in ("dsa", "gdba") and int(best_every) > 0:
            eng.track_best(int(best_every), infinity)
        tracked = _maxsum_track(eng, algo, cycles, cost_every, best_every, infinity, devices)
        if int(until_quiescent) > 0:
            cycles, ended = _run_until_quiescent(eng, cycles, until_quiescent)
            curve = []
        else:
            curve, ended = _run_and_trace(eng, algo, cycles, 0 if tracked else cost_every, infinity), {}  # (tracked: ONE run call)
        idx, _ = eng.assignment()
        extra = {**_dba_end(eng, algo), **ended}
        best = (_dsa_best(eng, algo, restarts, best_every, infinity) or _mgm_best(eng, algo, restarts, infinity)
                or _dba_best(eng, algo, restarts))
        if tracked:
            curve, best = _maxsum_result(eng, cycles, cost_every, best_every, infinity)
        if best:
            idx, more = best
            extra.update(more)
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
    _check_restarts(algo, restarts, best_every, draws, dba_stop)
    _check_maxsum_tracking(algo, cost_every, best_every, devices)
    _check_until_quiescent(algo, until_quiescent, devices)
    algo_kw = _algo_kw(algo, variant, probability, p_mode, seed, threshold, favor, modifier, violation, increase_mode,
                       dba_infinity, max_distance, restarts, draws, best_every, dba_stop)
    with _engine_for(graph, params, device, devices, lib_path, algo, algo_kw) as eng:
        if algo in ("dsa", "gdba") and int(best_every) > 0:
            eng.track_best(int(best_every), infinity)
        tracked = _maxsum_track(eng, algo, cycles, cost_every, best_every, infinity, devices)
        if int(until_quiescent) > 0:
            cycles, ended = _run_until_quiescent(eng, cycles, until_quiescent)
            curve = []
        else:
            curve, ended = _run_and_trace(eng, algo, cycles, 0 if tracked else cost_every, infinity), {}  # (tracked: ONE run call)
        idx, _ = eng.assignment()
        extra = {**_dba_end(eng, algo), **ended}
        best = (_dsa_best(eng, algo, restarts, best_every, infinity) or _mgm_best(eng, algo, restarts, infinity)
                or _dba_best(eng, algo, restarts))
        if tracked:
            curve, best = _maxsum_result(eng, cycles, cost_every, best_every, infinity)
        if best:
            idx, more = best
            extra.update(more)
        cost, violation = eng.eval_cost(idx, infinity=infinity) if best else eng.eval_cost(infinity=infinity)
    if graph.var_names is not None and graph.domains is not None:
        assignment = assignment_to_values(graph, idx)
    else:
        assignment = {f"v{i}": int(x) for i, x in enumerate(idx)}
    return {"assignment": assignment, "cost": cost, "violation": violation, "cycle": cycles,
            "cost_curve": curve, **extra}


def solve_dcop_dpop(dcop, *, precision: str = "f64", infinity: float = 10000, device: int = 0, max_bytes: int = 0,
                    lib_path: Optional[str] = None) -> Dict:
    """DPOP (pydcop/algorithms/dpop.py): the exact optimum, on the pseudo-tree the reference builds for the DCOP
    (pydcop_amd/computations_graph/pseudotree_fast.py) and compiled as the dpop_gpu plug-in compiles it -- the
    assignment `pydcop solve --algo dpop` returns.  Same result keys as `solve_dcop`; "cycle" is 0."""
    from . import plugin
    plugin.install()
    from pydcop.computations_graph import pseudotree_fast
    from pydcop_amd.algorithms.dpop_gpu import compile_pseudotree
    from .dpop import DpopEngine
    graph, tree = compile_pseudotree(pseudotree_fast.build_computation_graph(dcop).nodes)
    with DpopEngine(graph, Params(mode=dcop.objective, dtype=precision), tree=tree, max_bytes=max_bytes,
                    device=device, lib_path=lib_path) as eng:
        eng.solve()
        idx, _ = eng.assignment()
    assignment = assignment_to_values(graph, idx)
    violation, cost = dcop.solution_cost(assignment, infinity)
    return {"assignment": assignment, "cost": cost, "violation": violation, "cycle": 0, "cost_curve": []}


def solve_flat_dpop(graph: FlatGraph, objective: str = "min", *, precision: str = "f64", infinity: float = 10000,
                    device: int = 0, max_bytes: int = 0, lib_path: Optional[str] = None) -> Dict:
    """`solve_dcop_dpop` for a compiled instance: the tree is `build_pseudotree` over the instance's variable
    and factor order; cost and violations are evaluated by the engine."""
    from .dpop import DpopEngine
    with DpopEngine(graph, Params(mode=objective, dtype=precision), max_bytes=max_bytes, device=device,
                    lib_path=lib_path) as eng:
        eng.solve()
        idx, _ = eng.assignment()
        cost, violation = eng.eval_cost(infinity=infinity)
    if graph.var_names is not None and graph.domains is not None:
        assignment = assignment_to_values(graph, idx)
    else:
        assignment = {f"v{i}": int(x) for i, x in enumerate(idx)}
    return {"assignment": assignment, "cost": cost, "violation": violation, "cycle": 0, "cost_curve": []}


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
    kinds = {"damping": float, "stability": float, "noise": float, "seed": int,
             "damping_nodes": str, "start_messages": str, "precision": str, "devices": int,
             "variant": str, "probability": float, "p_mode": str, "threshold": float, "favor": str,
             "modifier": str, "violation": str, "increase_mode": str, "infinity": int, "max_distance": int,
             "restarts": int, "best_every": int, "draws": str, "dba_stop": str}
    kw = {}
    for item in args.algo_params:
        name, _, value = item.partition(":")
        if name not in kinds:
            raise SystemExit(f"Error: unknown parameter {name!r} (one of {sorted(kinds)})")
        kw[name] = kinds[name](value)
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
        if args.algo not in ("dsa", "mgm", "mgm2", "gdba", "dba"):
            kw.pop("seed", None)
        if args.algo == "dpop":
            res = solve_flat_dpop(graph, header.get("objective", "min"), infinity=args.infinity,
                                  precision=kw.get("precision", "f64"))
        else:
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
