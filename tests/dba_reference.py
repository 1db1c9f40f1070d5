"""The reference's own DbaComputation objects (pydcop/algorithms/dba.py) under keyed draws -- TEST
INFRASTRUCTURE ONLY, built like tests/gdba_reference.py."""
from collections import deque

from oracle.ref_harness import dsa_uniform, install_shims


def run_reference_dba(dcop, rounds, infinity=10000, max_distance=50, seed=0, var_index=None):
    """At most `rounds` rounds, FIFO delivery from ONE queue (both phases park early messages, so any
    order gives the same result).  Under FIFO the queue is a sequence of generations -- all `dba_ok` of a
    round, then all its `dba_improve`, then the `dba_ok` of the next -- and the messages sent while one
    generation is handled form the next.  The run ends with the first round in which a stop condition
    holds (tests/dba_oracle.py, Stop): once a computation has called `finished`, the generation being
    handled is still delivered to its end -- every other variable does that round's `_send_ok` -- and
    everything sent during it (the `dba_ok` of the next round, those of the variables that were handled
    before the stopper included, and `dba_end`) is dropped, as is whatever is sent afterwards.
    So is every message of a computation that has done `rounds` rounds (its `dba_ok` for the next one).
    For the duration of the run `pydcop.algorithms.dba.random` is a keyed object: choice(seq) =
    seq[int(u * len(seq))] over the sequence as given (domain order), u = dsa_uniform(seed,
    var_index[name], cycle, draw) with draw 8 at cycle 0 for the start value and draw 9 at the
    computation's cycle_count for one of the best values.
    Returns ({var: value}, {var: cost}, comps, info): info = {"moves", "stop_round" (0: none)}."""
    install_shims()
    from pydcop.algorithms import AlgorithmDef, ComputationDef, load_algorithm_module
    from pydcop.computations_graph import constraints_hypergraph as chg
    import pydcop.algorithms.dba as dba
    import logging

    names = sorted(dcop.variables) if var_index is None else None
    index = var_index or {n: i for i, n in enumerate(names)}
    ctx = {"comp": None, "moves": 0, "stop_round": 0}

    def instrumented(c):
        plain = c.value_selection

        def value_selection(val, cost=0):
            if c._mode != "starting" and val != c.current_value:
                ctx["moves"] += 1
            return plain(val, cost)

        def finished():
            if not ctx["stop_round"]:
                ctx["stop_round"] = c.cycle_count
        c.value_selection = value_selection
        c.finished = finished                       # (no agent to tell)

    class _Keyed:
        def __getattr__(self, name):
            import random as _r
            return getattr(_r, name)

        @staticmethod
        def choice(seq):
            c = ctx["comp"]
            seq = list(seq)
            if c._mode == "starting":
                u = dsa_uniform(seed, index[c.name], 0, 8)
            else:
                assert c._mode == "ok", c._mode
                u = dsa_uniform(seed, index[c.name], c.cycle_count, 9)
            return seq[int(u * len(seq))]

    saved, saved_inf = dba.random, dba.INFINITY
    dba.random = _Keyed()
    logging.disable(logging.CRITICAL)
    try:
        cg = chg.build_computation_graph(dcop)
        algo = AlgorithmDef.build_with_default_param(
            "dba", {"infinity": infinity, "max_distance": max_distance}, mode=dcop.objective)
        module = load_algorithm_module("dba")
        comps, nxt = {}, deque()

        def sender(src, dest, msg, prio=None, on_error=None):
            if ctx["stop_round"] or comps[src].cycle_count >= rounds:
                return
            nxt.append((src, dest, msg))

        for node in cg.nodes:
            c = module.build_computation(ComputationDef(node, algo))
            c.message_sender = sender
            instrumented(c)
            comps[node.name] = c
        for c in comps.values():
            ctx["comp"] = c
            c.start()
        while nxt and not ctx["stop_round"]:
            q, nxt = nxt, deque()                   # one generation, in the order it was sent
            while q:
                s, d, m = q.popleft()
                ctx["comp"] = comps[d]
                comps[d].on_message(s, m, 0.0)
    finally:
        dba.random = saved
        dba.INFINITY = saved_inf
        logging.disable(logging.NOTSET)
    values = {v: comps[v].current_value for v in dcop.variables}
    costs = {v: comps[v].current_cost for v in dcop.variables}
    return values, costs, comps, {"moves": ctx["moves"], "stop_round": ctx["stop_round"]}


def reference_state(g, kw, rounds):
    """What tools/make_golden_dba.py records: the reference's state as arrays (tests/dba_oracle.py `state()`,
    -1 / 0 where the reference holds None), every slot's weight, and {"moves", "stop_round", "rounds"}."""
    import numpy as np
    from oracle import ref_harness
    dcop, _ = ref_harness.flat_to_dcop(g, "min")
    index = {n: i for i, n in enumerate(g.var_names)}
    vals, costs, comps, info = run_reference_dba(dcop, rounds, var_index=index, **kw)
    doms = g.domains or [list(range(int(d))) for d in g.dom_size]
    cs = [comps[n] for n in g.var_names]
    ref = {"idx": np.array([doms[i].index(vals[n]) for i, n in enumerate(g.var_names)], dtype=np.int32),
           "has_cost": np.array([costs[n] is not None for n in g.var_names], dtype=np.uint8),
           "cost": np.array([0 if costs[n] is None else costs[n] for n in g.var_names], dtype=np.int32),
           "improve": np.array([c._my_improve for c in cs], dtype=np.int32),
           "new": np.array([-1 if c._new_value is None else doms[i].index(c._new_value) for i, c in enumerate(cs)],
                           dtype=np.int32),
           "counter": np.array([c._termination_counter for c in cs], dtype=np.int32),
           "consistent": np.array([bool(c._consistent) for c in cs], dtype=np.uint8)}
    # current_eval is a local of improve(): it is the held cost unless the variable moved afterwards
    # (value_selection(new, __cost__ - improve): then it is the held cost + the improvement)
    moved = np.array([bool(c._can_move) for c in cs])
    ref["eval"] = np.where(moved, ref["cost"] + ref["improve"], ref["cost"]).astype(np.int32)
    weights = []
    for i, c in enumerate(cs):
        assert len(c.__constraints_weights__) == int(g.var_rowptr[i + 1] - g.var_rowptr[i])
        weights += list(c.__constraints_weights__)
    played = [c for c in cs if c.neighbors]
    done = info["stop_round"] or rounds
    assert all(c.cycle_count == done for c in played), "the computations are not in lock step"
    return ref, np.array(weights, dtype=np.int32), dict(info, rounds=done)
