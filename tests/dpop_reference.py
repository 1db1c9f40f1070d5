"""The reference's own DpopAlgo objects (pydcop/algorithms/dpop.py) on the reference's own pseudo-tree, driven
in-process -- TEST INFRASTRUCTURE ONLY, built like tests/mgm2_reference.py.  A DpopAlgo joins its children's
UTILs in the order they arrive; here a parent gets them once all are there, in its `children` list order."""
import sys
from collections import deque

from oracle.ref_harness import install_shims


def reference_tree(dcop):
    """pseudotree.build_computation_graph -> (graph, {name: (parent, pseudo_parents, children, pseudo_children)})"""
    install_shims()
    from pydcop.computations_graph import pseudotree
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))     # (two frames per level of the tree)
    cg = pseudotree.build_computation_graph(dcop)
    return cg, {n.name: pseudotree.get_dfs_relations(n) for n in cg.nodes}


def run_reference_dpop(dcop, cg=None):
    """-> ({var: value}, {var: cost}, {var: ([dimension names], ndarray)} the UTIL every non-root sent, relations)"""
    install_shims()
    import logging
    import numpy as np
    from pydcop.algorithms import AlgorithmDef, ComputationDef, load_algorithm_module
    if cg is None:
        cg, rel = reference_tree(dcop)
    else:
        from pydcop.computations_graph.pseudotree import get_dfs_relations
        rel = {n.name: get_dfs_relations(n) for n in cg.nodes}
    logging.disable(logging.CRITICAL)
    try:
        algo = AlgorithmDef.build_with_default_param("dpop", {}, mode=dcop.objective)
        module = load_algorithm_module("dpop")
        comps, q, utils, waiting = {}, deque(), {}, {}

        def sender(src, dest, msg, prio=None, on_error=None):
            q.append((src, dest, msg))

        for node in cg.nodes:
            c = module.build_computation(ComputationDef(node, algo))
            c.message_sender = sender
            c._on_finished = lambda *a, **k: None   # (no agent to tell)
            comps[node.name] = c
        for c in comps.values():
            c.start()
        while q:
            s, d, m = q.popleft()
            if m.type != "UTIL":
                comps[d].on_message(s, m, 0.0)
                continue
            utils[s] = ([v.name for v in m.content.dimensions], np.array(m.content._m, dtype=np.float64))
            box = waiting.setdefault(d, {})
            box[s] = m
            children = rel[d][2]
            if len(box) == len(children):
                for c in children:
                    comps[d].on_message(c, box[c], 0.0)
    finally:
        logging.disable(logging.NOTSET)
    values = {v: comps[v].current_value for v in dcop.variables}
    costs = {v: comps[v].current_cost for v in dcop.variables}
    assert all(x is not None for x in values.values()), "a computation did not finish"
    return values, costs, utils, rel
