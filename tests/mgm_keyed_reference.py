"""The reference's own MgmComputation objects (pydcop/algorithms/mgm.py) under keyed draws -- TEST INFRASTRUCTURE
ONLY, built like tests/gdba_reference.py."""
from collections import deque

from oracle.ref_harness import dsa_uniform, install_shims


def run_reference_mgm_keyed(dcop, rounds, seed=0, var_index=None):
    """Exactly `rounds` rounds of (values, gains, decision): stop_cycle = rounds + 1 (mgm.py:407-411), FIFO delivery
    (MGM parks early messages, so any order gives the same result).  For the duration of the run
    `pydcop.algorithms.mgm.random` is a keyed object: choice(seq) = seq[int(u * len(seq))] over the sequence as
    given (domain order), u = dsa_uniform(seed, var_index[name], cycle, draw) with draw 10 at cycle 0 for the start
    value and draw 11 at the computation's cycle_count for one of the best values (tests/mgm_keyed_oracle.py);
    random() -- the number `_send_gain` attaches, which nothing reads -- is 0.  `var_index`: the variable's index
    in the keys, by default its position among the sorted names.
    Returns ({var: value}, {var: cost}, comps, the cycle_counts the draws of id 11 were made at)."""
    install_shims()
    from pydcop.algorithms import AlgorithmDef, ComputationDef, load_algorithm_module
    from pydcop.computations_graph import constraints_hypergraph as chg
    import pydcop.algorithms.mgm as mgm
    import logging

    names = sorted(dcop.variables) if var_index is None else None
    index = var_index or {n: i for i, n in enumerate(names)}
    ctx = {"comp": None, "start": False, "cycles": []}

    class _Keyed:
        def __getattr__(self, name):
            import random as _r
            return getattr(_r, name)

        @staticmethod
        def choice(seq):
            c = ctx["comp"]
            seq = list(seq)
            if ctx["start"]:
                u = dsa_uniform(seed, index[c.name], 0, 10)
            else:
                assert c._state == "values", c._state
                ctx["cycles"].append(c.cycle_count)
                u = dsa_uniform(seed, index[c.name], c.cycle_count, 11)
            return seq[int(u * len(seq))]

        @staticmethod
        def random():
            return 0.0

    saved = mgm.random
    mgm.random = _Keyed()
    logging.disable(logging.CRITICAL)
    try:
        cg = chg.build_computation_graph(dcop)
        algo = AlgorithmDef.build_with_default_param("mgm", {"stop_cycle": rounds + 1}, mode=dcop.objective)
        module = load_algorithm_module("mgm")
        comps, q = {}, deque()

        def sender(src, dest, msg, prio=None, on_error=None):
            q.append((src, dest, msg))

        for node in cg.nodes:
            c = module.build_computation(ComputationDef(node, algo))
            c.message_sender = sender
            c._on_finished = lambda *a, **k: None   # (no agent to tell)
            comps[node.name] = c
        ctx["start"] = True
        for c in comps.values():
            ctx["comp"] = c
            c.start()
        ctx["start"] = False
        while q:
            s, d, m = q.popleft()
            ctx["comp"] = comps[d]
            comps[d].on_message(s, m, 0.0)
    finally:
        mgm.random = saved
        logging.disable(logging.NOTSET)
    values = {v: comps[v].current_value for v in dcop.variables}
    costs = {v: comps[v].current_cost for v in dcop.variables}
    return values, costs, comps, ctx["cycles"]


def reference_state(g, mode, seed, rounds):
    """What tools/make_golden_mgm_keyed.py records: the reference's values and held costs as arrays (NaN: None)."""
    import numpy as np
    from oracle import ref_harness
    dcop, _ = ref_harness.flat_to_dcop(g, mode)
    index = {n: i for i, n in enumerate(g.var_names)}
    vals, costs, comps, cycles = run_reference_mgm_keyed(dcop, rounds, seed=seed, var_index=index)
    doms = g.domains or [list(range(int(d))) for d in g.dom_size]
    ref = {"idx": np.array([doms[i].index(vals[n]) for i, n in enumerate(g.var_names)], dtype=np.int32),
           "cost": np.array([np.nan if costs[n] is None else float(costs[n]) for n in g.var_names])}
    viol, cost = dcop.solution_cost(vals, float("inf"))
    return ref, cycles, (cost, viol)
