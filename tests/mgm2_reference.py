"""The reference's own Mgm2Computation objects (pydcop/algorithms/mgm2.py) under keyed draws -- TEST
INFRASTRUCTURE ONLY, built like oracle.ref_harness.run_reference_dsa (which it imports, unchanged)."""
from collections import deque

from oracle.ref_harness import dsa_uniform, install_shims


def run_reference_mgm2(dcop, rounds, threshold=0.5, favor="unilateral", seed=0, var_index=None):
    """Exactly `rounds` rounds (stop_cycle = rounds + 1: `_send_value` calls new_cycle() before the
    stop test), FIFO delivery (every phase parks early messages, so any order gives the same
    result).  For the duration of the run `pydcop.algorithms.mgm2.random` is a keyed object: the
    draw id comes from the computation's `_state` and from what the sequence holds, the sequence is
    put in the canonical order of tests/mgm2_oracle.py, and every draw is
    dsa_uniform(seed, var_index[name], cycle, draw).  Returns ({var: value}, {var: cost}, comps)."""
    install_shims()
    from pydcop.algorithms import AlgorithmDef, ComputationDef, load_algorithm_module
    from pydcop.computations_graph import constraints_hypergraph as chg
    from pydcop.dcop.objects import Variable
    import pydcop.algorithms.mgm2 as mgm2
    import logging

    names = sorted(dcop.variables) if var_index is None else None
    index = var_index or {n: i for i, n in enumerate(names)}
    ctx = {"comp": None}

    def u(draw):
        c = ctx["comp"]
        cycle = 0 if c._state is None else c.cycle_count
        return dsa_uniform(seed, index[c.name], cycle, draw)

    class _Keyed:
        def __getattr__(self, name):
            import random as _r
            return getattr(_r, name)

        @staticmethod
        def uniform(a, b):
            state = ctx["comp"]._state
            assert state in ("value", "offer"), state
            return a + (b - a) * u(1 if state == "value" else 4)

        @staticmethod
        def choice(seq):
            c = ctx["comp"]
            seq = list(seq)
            if c._state is None:                                     # on_start: values, domain order
                return seq[int(u(0) * len(seq))]
            if c._state == "value":
                if isinstance(seq[0], Variable):                     # partner: graph index order
                    seq = sorted(seq, key=lambda v: index[v.name])
                    return seq[int(u(2) * len(seq))]
                return seq[int(u(3) * len(seq))]                     # best values: domain order
            assert c._state == "offer", c._state                     # (val_p, my_val, offerer)
            dom = {n.name: list(n.domain) for n in c._neighbors}
            mine = list(c.variable.domain)
            seq = sorted(seq, key=lambda t: (index[t[2]], dom[t[2]].index(t[0]), mine.index(t[1])))
            return seq[int(u(5) * len(seq))]

    saved = mgm2.random
    mgm2.random = _Keyed()
    logging.disable(logging.CRITICAL)
    try:
        cg = chg.build_computation_graph(dcop)
        algo = AlgorithmDef.build_with_default_param(
            "mgm2", {"stop_cycle": rounds + 1, "threshold": threshold, "favor": favor}, mode=dcop.objective)
        module = load_algorithm_module("mgm2")
        comps, q = {}, deque()

        def sender(src, dest, msg, prio=None, on_error=None):
            q.append((src, dest, msg))

        for node in cg.nodes:
            c = module.build_computation(ComputationDef(node, algo))
            c.message_sender = sender
            c._on_finished = lambda *a, **k: None   # (no agent to tell)
            comps[node.name] = c
        for c in comps.values():
            ctx["comp"] = c
            c.start()
        while q:
            s, d, m = q.popleft()
            ctx["comp"] = comps[d]
            comps[d].on_message(s, m, 0.0)
    finally:
        mgm2.random = saved
        logging.disable(logging.NOTSET)
    values = {v: comps[v].current_value for v in dcop.variables}
    costs = {v: comps[v].current_cost for v in dcop.variables}
    return values, costs, comps
