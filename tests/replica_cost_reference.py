"""The solution cost of an assignment from the FlatGraph arrays alone, in plain Python: what the device cost of the
replica engines (k_cost_partial / k_cost_final, pydcop_amd/csrc/replica_cost.h) and the engines' host eval_cost are
checked against.  No call into any library build.

Items: the constraints in index order, then the variables.  A constraint's entry is indexed row-major over its scope;
with Params(dtype="f32") the tables are the narrowed ones (float32 and back), as the device documents
(include/maxsum_gpu.h, mxs_*_replica_costs).  The variable part is eval_var_cost where the graph has one, else
var_cost, never narrowed.  An item equal to `infinity` is a violation and left out of the sum.

The bound: the device adds n items in f64 in a fixed order of its own (runs of 4, a tree over 256 threads, the
partials in index order), the host adds them one after another.  For ANY order of n floating-point additions
|computed - exact| <= gamma(n - 1) * sum |item|, gamma(k) = k u / (1 - k u), u = 2**-53 (Higham, Accuracy and
Stability of Numerical Algorithms, section 4.2).  `cost` is math.fsum of the items, the exact sum rounded once."""
import math

import numpy as np

INF = float("inf")
U = 2.0 ** -53
CHUNK, RUN = 1024, 4          # the items of one block and of one thread of k_cost_partial


def reference_items(graph, params, idx, infinity=INF):
    """every item of the assignment `idx` (graph order) as a Python float, violations included"""
    tables = graph.tables
    if params.dtype == "f32":
        tables = tables.astype(np.float32).astype(np.float64)
    tables, dom = tables.tolist(), graph.dom_size.tolist()
    rowptr, scope, toff = graph.factor_rowptr.tolist(), graph.edge_var.tolist(), graph.table_off.tolist()
    idx = [int(x) for x in idx]
    assert len(idx) == graph.n_vars and all(0 <= idx[v] < dom[v] for v in range(graph.n_vars))
    items = []
    for f in range(graph.n_factors):
        lin = 0
        for k in range(rowptr[f], rowptr[f + 1]):
            lin = lin * dom[scope[k]] + idx[scope[k]]
        items.append(tables[toff[f] + lin])
    own = (graph.eval_var_cost if graph.eval_var_cost is not None else graph.var_cost).tolist()
    off = 0
    for v in range(graph.n_vars):
        items.append(own[off + idx[v]])
        off += dom[v]
    return items


def reference_cost(graph, params, idx, infinity=INF):
    """-> (cost, violations, sum_abs, items): math.fsum of the items that are not `infinity`, how many are, math.fsum
    of the magnitudes of the summed ones, the number of items"""
    items = reference_items(graph, params, idx, infinity)
    soft = [x for x in items if x != infinity]
    return math.fsum(soft), len(items) - len(soft), math.fsum(abs(x) for x in soft), len(items)


def cost_bound(items, sum_abs):
    """gamma(items - 1) * sum_abs: the error of any summation order of `items` numbers"""
    k = max(items - 1, 0) * U
    return k * sum_abs / (1.0 - k)


def is_exact(graph, params):
    """integer tables and no variable costs: every partial sum is an integer far below 2**53, any order gives the
    same bits"""
    own = graph.eval_var_cost if graph.eval_var_cost is not None else graph.var_cost
    return bool((graph.tables == np.floor(graph.tables)).all() and np.abs(graph.tables).max(initial=0) < 2 ** 24
                and not own.any())


def assert_chunks_carry_weight(graph, params, idx, infinity=INF, runs=True):
    """(the reference side) the sum of every 1024-item chunk -- a block's partial -- and, with `runs`, of every 4-item
    run -- a thread's -- is at least 1000 times the bound in magnitude: a dropped, doubled or misplaced one cannot
    hide inside the bound"""
    items = [0.0 if x == infinity else x for x in reference_items(graph, params, idx, infinity)]
    floor = 1000.0 * cost_bound(len(items), math.fsum(abs(x) for x in items))
    for size in (CHUNK, RUN) if runs else (CHUNK,):
        for i in range(0, len(items), size):
            s = math.fsum(items[i:i + size])
            assert abs(s) >= floor and s != 0.0, f"items {i}..{i + size - 1} sum to {s!r}, the bound is {floor / 1000.0!r}"


def assert_chunks_hold_violations(graph, params, idx, infinity):
    """(the reference side) every 1024-item chunk that holds a constraint holds a violation.  (A chunk of variables
    alone cannot on these instances: they have no variable costs.)"""
    items = reference_items(graph, params, idx, infinity)
    for i in range(0, graph.n_factors, CHUNK):
        assert any(x == infinity for x in items[i:i + CHUNK]), f"no violation among the items {i}..{i + CHUNK - 1}"


def acceptable_winners(refs, is_max, exact):
    """refs: per replica (cost, violations, sum_abs, items, idx).  -> (w, ok): w the lexicographic minimum of
    (violations, cost -- negated in max mode --, index); ok: w and, unless `exact`, every replica of as many
    violations and ANOTHER assignment whose cost lies within the two bounds of w's -- a sum in another order may rank
    those two either way.  (The same assignment gives the same bits: there the lowest index wins.)"""
    n = len(refs)
    w = min(range(n), key=lambda r: (refs[r][1], -refs[r][0] if is_max else refs[r][0], r))
    ok = {w}
    if not exact:
        for r in range(n):
            near = cost_bound(refs[r][3], refs[r][2]) + cost_bound(refs[w][3], refs[w][2])
            if (r != w and refs[r][1] == refs[w][1] and abs(refs[r][0] - refs[w][0]) <= near
                    and not np.array_equal(refs[r][4], refs[w][4])):
                ok.add(r)
    return w, ok


def check_replica_costs(eng, replicas, infinity=INF, cost=None, viol=None):
    """the engine's device costs (replica_costs; or the `cost`, `viol` it returned) of the replicas `replicas` against
    reference_cost of their assignments: violations exactly, the cost within cost_bound -- exactly where is_exact;
    in f64 mode the engine's host eval_cost the same way.  -> {replica: (cost, violations, sum_abs, items, idx)}"""
    if cost is None:
        cost, viol = eng.replica_costs(infinity)
    graph, params = eng.graph, eng.params
    exact = is_exact(graph, params)
    out = {}
    for r in replicas:
        idx = eng.assignment(r)[0]
        ref = reference_cost(graph, params, idx, infinity)
        out[r] = ref + (idx,)
        bound = 0.0 if exact else cost_bound(ref[3], ref[2])
        assert int(viol[r]) == ref[1], f"replica {r}: {int(viol[r])} violations on the device, {ref[1]} by the reference"
        assert abs(float(cost[r]) - ref[0]) <= bound, \
            f"replica {r}: device cost {float(cost[r])!r}, reference {ref[0]!r}, bound {bound!r}"
        if params.dtype == "f64":
            c, v = eng.eval_cost(idx, infinity)
            assert v == ref[1], f"replica {r}: {v} violations by the host, {ref[1]} by the reference"
            assert abs(c - ref[0]) <= bound, f"replica {r}: host cost {c!r}, reference {ref[0]!r}, bound {bound!r}"
    return out
