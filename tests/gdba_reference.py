"""The reference's own GdbaComputation objects (pydcop/algorithms/gdba.py) under keyed draws -- TEST
INFRASTRUCTURE ONLY, built like tests/mgm2_reference.py."""
from collections import deque

from oracle.ref_harness import dsa_uniform, install_shims


def run_reference_gdba(dcop, rounds, modifier="A", violation="NZ", increase_mode="E", seed=0, var_index=None):
    """Exactly `rounds` rounds, FIFO delivery (both phases park early messages, so any order gives
    the same result).  The reference has no stop condition: a computation that has decided round
    `rounds` (its cycle_count is then rounds + 1) gets no hearing for its next `gdba_ok`, which is
    dropped where it is sent.  For the duration of the run `pydcop.algorithms.gdba.random` is a keyed
    object: choice(seq) = seq[int(u * len(seq))] over the sequence as given (domain order), u =
    dsa_uniform(seed, var_index[name], cycle, draw) with draw 6 at cycle 0 for the start value and
    draw 7 at the computation's cycle_count for one of the best values (tests/gdba_oracle.py).
    Returns ({var: value}, {var: cost}, comps, number of moves made after the start)."""
    install_shims()
    from pydcop.algorithms import AlgorithmDef, ComputationDef, load_algorithm_module
    from pydcop.computations_graph import constraints_hypergraph as chg
    import pydcop.algorithms.gdba as gdba
    import logging

    names = sorted(dcop.variables) if var_index is None else None
    index = var_index or {n: i for i, n in enumerate(names)}
    ctx = {"comp": None, "moves": 0}

    def counted(c):
        plain = c.value_selection

        def value_selection(val, cost=0):
            if c._waiting_mode != "starting" and val != c.current_value:
                ctx["moves"] += 1
            return plain(val, cost)
        c.value_selection = value_selection

    class _Keyed:
        def __getattr__(self, name):
            import random as _r
            return getattr(_r, name)

        @staticmethod
        def choice(seq):
            c = ctx["comp"]
            seq = list(seq)
            if c._waiting_mode == "starting":
                u = dsa_uniform(seed, index[c.name], 0, 6)
            else:
                assert c._waiting_mode == "ok", c._waiting_mode
                u = dsa_uniform(seed, index[c.name], c.cycle_count, 7)
            return seq[int(u * len(seq))]

    saved = gdba.random
    gdba.random = _Keyed()
    logging.disable(logging.CRITICAL)
    try:
        cg = chg.build_computation_graph(dcop)
        algo = AlgorithmDef.build_with_default_param(
            "gdba", {"modifier": modifier, "violation": violation, "increase_mode": increase_mode}, mode=dcop.objective)
        module = load_algorithm_module("gdba")
        comps, q = {}, deque()

        def sender(src, dest, msg, prio=None, on_error=None):
            if comps[src].cycle_count > rounds:
                return
            q.append((src, dest, msg))

        for node in cg.nodes:
            c = module.build_computation(ComputationDef(node, algo))
            c.message_sender = sender
            c._on_finished = lambda *a, **k: None   # (no agent to tell)
            counted(c)
            comps[node.name] = c
        for c in comps.values():
            ctx["comp"] = c
            c.start()
        while q:
            s, d, m = q.popleft()
            ctx["comp"] = comps[d]
            comps[d].on_message(s, m, 0.0)
    finally:
        gdba.random = saved
        logging.disable(logging.NOTSET)
    values = {v: comps[v].current_value for v in dcop.variables}
    costs = {v: comps[v].current_cost for v in dcop.variables}
    return values, costs, comps, ctx["moves"]


def reference_modifiers(comp, graph, slot_k, index):
    """The modifier table of the computation's k-th constraint under the keys its look-ups use (assignments of
    the constraint's own scope), in the layout of the constraint's table -- what the engine stores for a live
    slot; in mode T every entry holds the same counter."""
    import itertools
    import numpy as np
    rel = comp.constraints[slot_k][0]
    mods = comp.__constraints_modifiers__[rel]
    dims = rel.dimensions
    out = []
    for combo in itertools.product(*[list(d.domain) for d in dims]):
        asgt = {d.name: x for d, x in zip(dims, combo)}      # (a repeated variable: the last position wins,
        key = frozenset(asgt.items())                        #  such entries are never read)
        out.append(mods[key] if key in mods else mods.default_factory())
    return np.array(out, dtype=np.int64)


def reference_state(g, mode, kw, rounds):
    """What tools/make_golden_gdba.py records: the reference's state as arrays, and its number of moves."""
    import numpy as np
    from oracle import ref_harness
    dcop, _ = ref_harness.flat_to_dcop(g, mode)
    index = {n: i for i, n in enumerate(g.var_names)}
    vals, costs, comps, moves = run_reference_gdba(dcop, rounds, var_index=index, **kw)
    doms = g.domains or [list(range(int(d))) for d in g.dom_size]
    nV = g.n_vars
    ref = {"idx": np.array([doms[i].index(vals[n]) for i, n in enumerate(g.var_names)], dtype=np.int32),
           "cost": np.array([np.nan if costs[n] is None else float(costs[n]) for n in g.var_names]),
           "improve": np.array([float(comps[n]._my_improve) for n in g.var_names])}
    ref["new"] = np.array([ref["idx"][i] if comps[n]._new_value is None else doms[i].index(comps[n]._new_value)
                           for i, n in enumerate(g.var_names)], dtype=np.int32)
    mods = []
    for i, n in enumerate(g.var_names):
        for k in range(int(g.var_rowptr[i + 1] - g.var_rowptr[i])):
            mods.append(reference_modifiers(comps[n], g, k, index))
    played = [c for c in comps.values() if c.neighbors]
    assert all(c.cycle_count == rounds + 1 for c in played)          # lock-step: cycle_count 13 after 12 rounds
    viol, cost = dcop.solution_cost(vals, float("inf"))
    return ref, mods, moves, (cost, viol)
