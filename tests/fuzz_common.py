"""Random instances through an engine build and its oracle, bit for bit.

`instance(seed)` (domains 1..17, arities 1..4, both modes, both precisions, every start_messages /
damping_nodes choice, random layout flags) feeds the Max-Sum sweep (`fuzz_maxsum`) and asynchronous Max-Sum,
DSA and MGM (`fuzz_others`).  `local_instance(seed)` (3..60 or 65..200 variables: a full wave, a second and a
third block of the thread-per-variable kernels; two or three unequal domain sizes in one graph) feeds MGM-2,
GDBA and DBA (`fuzz_mgm2`, `fuzz_gdba`, `fuzz_dba`), `dpop_instance(seed)` (4..40 variables, sparse, forests,
one-value variables, the caller's own tree every fourth seed) feeds DPOP (`fuzz_dpop`).  `replica_instance(seed)`
(local_instance, every third seed 260..520 variables; 1..66 replicas) feeds the replica engines -- DSA, MGM with
keyed draws, MGM-2 -- with their device costs and their ranking (`fuzz_replicas`); `gdba_replica_instance(seed)` and
`dba_replica_instance(seed)` (the recipes of gdba_instance / dba_instance at those sizes and replica counts, on
streams of their own) feed GDBA and DBA as replicas: modifier tables, device costs and ranking; weights, both stop
policies, stop rounds, violations, ranking and the per-replica "no best value" error (`fuzz_gdba_replicas`,
`fuzz_dba_replicas`).
`python tests/fuzz_common.py FIRST LAST` runs the seeds FIRST..LAST-1 of every driver on the emulated build;
tests/test_fuzz_emu.py runs a few of them in the CPU suite, tests/test_gpu_fuzz.py on the GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pydcop_amd import generators as G  # noqa: E402
from pydcop_amd.graph import Params  # noqa: E402


def instance(seed):
    rng = np.random.default_rng(1000 + seed)
    nv, nf = int(rng.integers(3, 60)), int(rng.integers(1, 120))
    # ($FUZZ_DOMS=big: ad-hoc sweeps over the domains of the round-5 kernels too -- lane grids of 16 / 64 lanes, box overhang)
    choices = [1, 2, 3, 4, 5, 7, 9, 17] if os.environ.get("FUZZ_DOMS") != "big" else [1, 2, 3, 4, 5, 6, 8, 9, 12, 17, 21, 24, 33]
    doms = tuple(int(x) for x in rng.choice(choices, size=int(rng.integers(1, 4))))
    max_arity = int(rng.integers(1, 5))
    if os.environ.get("FUZZ_DOMS") == "big" and max(doms) > 17:
        max_arity = min(max_arity, 3 if max(doms) <= 24 else 2)  # (keeps the emulated sweep's tables small)
    g = G.random_mixed(nv, nf, seed=seed, max_arity=max_arity, dom_choices=doms,
                       float_tables=bool(rng.integers(0, 2)))
    kw = dict(mode="max" if rng.integers(0, 2) else "min", dtype="f32" if rng.integers(0, 3) == 0 else "f64",
              start_messages=["leafs", "leafs_vars", "all"][int(rng.integers(0, 3))],
              damping_nodes=["vars", "factors", "both", "none"][int(rng.integers(0, 4))],
              damping=float(rng.choice([0.0, 0.3, 0.5])), stability=float(rng.choice([0.02, 0.1, 0.5])))
    flags = int(rng.choice([0, 0, 2048, 8192, 256, 16, 8, 2048 | 8192]))
    if os.environ.get("FUZZ_DOMS") == "big":  # (+ the round-5 switches: generic instead of lane grids, no pack8, pack8 in its own launch)
        flags |= int(rng.choice([0, 0, 0, 524288, 1048576, 2097152]))
    return g, kw, flags, rng


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what


def fuzz_maxsum(seed, lib_path):
    from oracle.maxsum_oracle import OracleMaxSum
    from pydcop_amd.engine import MaxSumEngine
    g, kw, flags, _ = instance(seed)
    with MaxSumEngine(g, Params(layout_flags=flags, **kw), lib_path=lib_path) as e:
        o = OracleMaxSum(g, Params(**kw))
        done = 0
        for n in (0, 1, 2, 5):
            e.run(n), o.run(n)
            done += n
            for a, b in zip(e.messages(), o.messages()):
                assert np.array_equal(a, b), f"messages after {done} cycles"
            _same(e.assignment(), o.assignment(), f"selection after {done} cycles")
        o.close()


def fuzz_others(seed, lib_path):
    from amaxsum_common import same_state
    from oracle.amaxsum_oracle import OracleAMaxSum
    from oracle.dsa_oracle import OracleDsa
    from oracle.mgm_oracle import OracleMgm
    from pydcop_amd.amaxsum import AMaxSumEngine
    from pydcop_amd.dsa import DsaEngine
    from pydcop_amd.mgm import MgmEngine
    g, kw, _, rng = instance(seed)
    e, o = AMaxSumEngine(g, Params(**kw), lib_path=lib_path), OracleAMaxSum(g, Params(**kw))
    for gens in (1, 2, 4, 7):
        if o.pending > 5000:
            break
        assert e.run(gens) == o.run(gens)
        same_state(e, o, f"generations < {gens}")
    e.close(), o.close()
    p = Params(mode=kw["mode"], dtype=kw["dtype"])
    dsa_kw = dict(variant="ABC"[int(rng.integers(0, 3))], probability=float(rng.choice([0.3, 0.7, 1.0])), seed=seed)
    for e, o, n in ((DsaEngine(g, p, lib_path=lib_path, **dsa_kw), OracleDsa(g, p, **dsa_kw), 6),
                    (MgmEngine(g, p, lib_path=lib_path), OracleMgm(g, p), 5)):
        e.run(n), o.run(n)
        _same(e.assignment(), o.assignment(), type(e).__name__)
        e.close(), o.close()


# ---- MGM-2, GDBA, DBA, DPOP ---------------------------------------------------------------------------
STEPS = (0, 1, 1, 3, 5)                  # the Python oracles dominate the run time: ten rounds in all
LOCAL_DOMS = (1, 2, 3, 4, 5, 8, 9, 17)
DBA_DOMS = (2, 3, 4, 5, 8, 9, 24, 32, 33, 64, 65)
DPOP_DOMS = (1, 2, 3, 4, 5, 7)
MAX_TABLE = 16_000                       # entries of one constraint table (and, over 32, words of a slot's bit rows)
DPOP_MAX_ENTRIES = 300_000
GDBA_STREAM = 22                         # of the streams 20..35 tried: every GDBA variant raises a modifier and moves within its two GPU seeds
DPOP_FACTORS = (0.8, 1.8)                # constraints per variable
GPU_SEEDS = {"mgm2": range(0, 48), "gdba": range(0, 48), "dba": range(0, 48), "dpop": range(0, 40),
             "replicas": range(0, 48), "gdba_replicas": range(0, 48),
             "dba_replicas": range(0, 48)}   # tests/test_gpu_fuzz.py


def local_instance(seed, dom_set=LOCAL_DOMS, slots=(0.8, 3.2), stream=20, n_vars=None):
    """-> (graph, rng).  Half the seeds 3..60 variables, the other half 65..200 (the halves alternate every 24
    seeds, so that a seed-indexed choice of period 24 meets both; `n_vars`: a range to draw from, of the seed's own
    stream, instead); two or three distinct domain sizes of
    `dom_set` in one graph; arities up to 3, up to 4 when every domain is 5 or less, fewer where a table would
    pass MAX_TABLE entries; `slots`: the range of constraints a variable is in, on average (or a function
    of the drawn domain sizes that gives it); `stream`: which random stream of the seed."""
    from mgm_common import shuffled_names, with_init
    rng = np.random.default_rng([seed, stream])
    big = (seed + seed // 24) % 2 == 1
    nv = int(rng.integers(65, 201)) if big else int(rng.integers(3, 61))
    if n_vars is not None:
        nv = int(np.random.default_rng([seed, stream, 1]).integers(n_vars[0], n_vars[1] + 1))
    doms = tuple(int(x) for x in rng.choice(dom_set, size=int(rng.integers(2, 4)), replace=False))
    top = max(doms)
    max_arity = int(rng.integers(2, 5 if top <= 5 else 4))
    while max_arity > 2 and top ** max_arity > MAX_TABLE:
        max_arity -= 1
    lo, hi = slots(doms) if callable(slots) else slots
    nf = max(1, int(nv * rng.uniform(lo, hi) / (0.5 * (1 + max_arity))))     # (arities 1..max_arity, equally likely)
    g = G.random_mixed(nv, nf, seed=int(rng.integers(0, 2 ** 31)), max_arity=max_arity, dom_choices=doms,
                       float_tables=bool(rng.integers(0, 2)))
    if rng.integers(0, 2):
        g = with_init(g, seed)
    if rng.integers(0, 2):
        g = shuffled_names(g, seed)
    return g, rng


def mgm2_instance(seed):
    """-> (graph, Params, MGM-2 kwargs)"""
    from mgm2_oracle import FAVORS
    g, rng = local_instance(seed)
    kw = dict(favor=FAVORS[int(rng.integers(0, 3))], threshold=float(rng.choice([0.0, 0.3, 0.5, 0.6, 1.0])), seed=seed)
    p = Params(mode="max" if rng.integers(0, 2) else "min", dtype="f32" if rng.integers(0, 3) == 0 else "f64")
    if rng.integers(0, 4) == 0:          # 0 / 1 tables: global gains tie with unilateral ones, `favor` decides
        g.tables = np.floor(g.tables) % 2
    return g, p, kw


def gdba_instance(seed, stream=GDBA_STREAM, n_vars=None):
    """-> (graph, Params, GDBA kwargs): the variant follows the seed, 24 consecutive seeds cover all 24"""
    import itertools
    from gdba_common import dyadic_var_costs
    from gdba_oracle import INCREASE_MODES, MODIFIERS, VIOLATIONS
    mod, vio, inc = list(itertools.product(MODIFIERS, VIOLATIONS, INCREASE_MODES))[seed % 24]
    g, rng = local_instance(seed, stream=stream, n_vars=n_vars)
    p = Params(mode="max" if rng.integers(0, 2) else "min", dtype="f32" if rng.integers(0, 3) == 0 else "f64")
    # the reference sums the variable costs in the order of a Python set: real-valued ones (random_mixed's) only in
    # mode T, as the pinned cases do (gdba_oracle.py, Determinism); dyadic ones or none elsewhere
    costs = int(rng.integers(0, 3 if inc == "T" else 2))
    if costs == 0:
        g.var_cost = np.zeros_like(g.var_cost)
    elif costs == 1:
        g = dyadic_var_costs(g, seed)
    return g, p, dict(modifier=mod, violation=vio, increase_mode=inc, seed=seed)


def dba_slots(doms, density, infinity):
    """How many constraints a variable of a DBA instance is in.  A value is free of violations with probability
    (1 - density)^k under k constraints: k = ln D / -ln(1 - density) leaves about one such value among D, the
    instances that are neither satisfied at once (the run stops, no weight ever rises) nor hopeless.  With
    `infinity: 2` two violated constraints already reach infinity, and a variable all of whose values meet
    three ends the run in round 1 ("no best value"): 0.4 k there, at most 4.5, about one at the highest density."""
    k = float(np.log(np.mean(doms)) / -np.log(1.0 - density))
    if infinity == 2:
        if density > 0.5:
            return 0.7, 1.5
        k = min(max(0.4 * k, 1.5), 4.5)
    else:
        k = min(max(k, 1.5), 8.0)
    return 0.75 * k, 1.25 * k


def dba_instance(seed, stream=20, pre_stream=(22,), n_vars=None):
    """-> (graph, Params, DBA kwargs): tables of 0 or c at a drawn violation density; (c, infinity) = (2, 2): an
    eval can EQUAL infinity; (1000, 999.5): ceil(infinity) differs from it"""
    pre = np.random.default_rng([seed, *pre_stream])
    c, infinity = [(1000.0, 1000), (1000.0, 999.5), (2.0, 2)][int(pre.integers(0, 3))]
    density = float(pre.choice([0.15, 0.5, 0.85]))
    g, rng = local_instance(seed, DBA_DOMS, slots=lambda doms: dba_slots(doms, density, infinity), stream=stream,
                            n_vars=n_vars)
    g.tables = c * (rng.random(g.tables.shape[0]) < density)
    g.var_cost = np.zeros_like(g.var_cost)
    return g, Params(), dict(infinity=infinity, max_distance=int(rng.choice([2, 3, 50])), seed=seed)


def keep_factors(g, n):
    """the graph with its first n constraints only"""
    from pydcop_amd.generators import _finish
    h = _finish(g.dom_size, g.var_cost, g.factor_rowptr[:n + 1].copy(), g.edge_var[:g.factor_rowptr[n]].copy(),
                g.tables[:g.table_off[n]].copy(), g.table_off[:n + 1].copy())
    h.var_names = g.var_names
    return h


def reversed_dfs_tree(g):
    """A pseudo-tree other than build_pseudotree's: per component a depth-first search from its variable of
    the highest index, the neighbours walked in reverse; every constraint's scope is a clique of the
    neighbour graph, and a depth-first tree keeps a clique on one root path."""
    from pydcop_amd.dpop import neighbor_lists, pack_tree
    nbrs = neighbor_lists(g)
    n = g.n_vars
    parent, children, seen = [-1] * n, [[] for _ in range(n)], [False] * n
    for root in range(n - 1, -1, -1):
        if seen[root]:
            continue
        seen[root] = True
        stack = [(root, iter(reversed(nbrs[root])))]
        while stack:
            v, it = stack[-1]
            u = next((u for u in it if not seen[u]), None)
            if u is None:
                stack.pop()
                continue
            seen[u] = True
            parent[u] = v
            children[v].append(u)
            stack.append((u, iter(reversed(nbrs[u]))))
    return pack_tree(parent, children)


def measure_tree(g, tree):
    """What the engine checks of a tree and sizes from it (dpop.h): parent and children lists consistent, every
    variable reached from a root, every scope on one root path -> (separators by variable, all UTIL entries)."""
    parent, crow, cidx = (np.asarray(a) for a in tree)
    n = g.n_vars
    assert len(parent) == n and len(crow) == n + 1 and len(cidx) == crow[-1]
    for v in range(n):
        assert all(parent[c] == v for c in cidx[crow[v]:crow[v + 1]])
    assert sorted(int(c) for c in cidx) == [v for v in range(n) if parent[v] >= 0]
    depth, order = np.zeros(n, dtype=np.int64), []
    stack = [r for r in range(n) if parent[r] < 0]
    while stack:
        v = stack.pop()
        order.append(v)
        for c in cidx[crow[v]:crow[v + 1]]:
            depth[c] = depth[v] + 1
            stack.append(int(c))
    assert len(order) == n, "a cycle"
    sep = [set() for _ in range(n)]
    for f in range(g.n_factors):
        scope = [int(u) for u in g.edge_var[g.factor_rowptr[f]:g.factor_rowptr[f + 1]]]
        low, path = max(scope, key=lambda u: depth[u]), set()
        a = low
        while a >= 0:
            path.add(a)
            a = int(parent[a])
        assert set(scope) <= path, f"the scope of constraint {f} does not lie on one root path"
        sep[low].update(scope)
    total = 0
    for v in reversed(order):
        sep[v].discard(v)
        if parent[v] >= 0:
            sep[parent[v]].update(sep[v])
            total += int(np.prod([int(g.dom_size[u]) for u in sep[v]], dtype=np.int64))
    return sep, total


def dpop_instance(seed):
    """-> (graph, Params, tree or None, shrink steps).  4..40 variables, about as many constraints (forests and
    variables without any among them), domains of DPOP_DOMS; every third seed integer tables on a few levels;
    every fourth seed a tree of its own.  While the UTILs hold more than DPOP_MAX_ENTRIES entries in all, the
    last quarter of the constraints goes: no seed is left out."""
    from dpop_common import int_ties
    from pydcop_amd.dpop import build_pseudotree
    rng = np.random.default_rng([seed, 21])
    nv = int(rng.integers(4, 41))
    nf = max(1, int(nv * rng.uniform(*DPOP_FACTORS)))
    doms = tuple(int(x) for x in rng.choice(DPOP_DOMS, size=int(rng.integers(2, 4)), replace=False))
    g = G.random_mixed(nv, nf, seed=int(rng.integers(0, 2 ** 31)), max_arity=int(rng.integers(2, 4)), dom_choices=doms,
                       float_tables=bool(rng.integers(0, 2)))
    p = Params(mode="max" if rng.integers(0, 2) else "min", dtype="f32" if rng.integers(0, 3) == 0 else "f64")
    if seed % 3 == 2:
        g = int_ties(g, 2 + seed % 2)
    own, shrinks = seed % 4 == 3, 0
    while True:
        tree = reversed_dfs_tree(g) if own else build_pseudotree(g)
        if measure_tree(g, tree)[1] <= DPOP_MAX_ENTRIES:
            return g, p, (tree if own else None), shrinks
        g = keep_factors(g, g.n_factors - max(1, g.n_factors // 4))
        shrinks += 1


def fuzz_mgm2(seed, lib_path, steps=STEPS):
    from mgm2_common import compare_mgm2
    from mgm2_oracle import OracleMgm2
    g, p, kw = mgm2_instance(seed)
    compare_mgm2(OracleMgm2, g, p, kw, lib_path=lib_path, steps=steps)


def fuzz_gdba(seed, lib_path, steps=STEPS):
    from gdba_common import compare_gdba
    from gdba_oracle import OracleGdba
    g, p, kw = gdba_instance(seed)
    compare_gdba(OracleGdba, g, p, kw, lib_path=lib_path, steps=steps)


def dba_failing_step(g, p, kw, steps=STEPS):
    """the index of the run call of `steps` in which the oracle raises IndexError (improve > 0 with no best
    value: every eval above infinity), None where it raises in none"""
    from dba_oracle import OracleDba
    o = OracleDba(g, p, **kw)
    for i, n in enumerate(steps):
        try:
            o.run(n)
        except IndexError:
            return i
    return None


def compare_dba_fallible(g, p, kw, lib_path=None, steps=STEPS):
    """compare_dba; where the oracle raises IndexError, the engine returns its "no best value" error in the
    same run call, and everything before that call is equal"""
    import pytest
    from dba_common import compare_dba, same_state
    from dba_oracle import OracleDba
    from pydcop_amd.dba import DbaEngine
    from pydcop_amd.engine import MaxSumGpuError
    bad = dba_failing_step(g, p, kw, steps)
    if bad is None:
        compare_dba(OracleDba, g, p, kw, lib_path=lib_path, steps=steps)
        return
    with DbaEngine(g, p, lib_path=lib_path, **kw) as eng:
        ora = OracleDba(g, p, **kw)
        assert eng.mask_bytes == ora.mask_bytes
        for n in steps[:bad]:
            eng.run(n), ora.run(n)
            same_state(eng, ora, f"after {ora.cycle_count} rounds")
        with pytest.raises(IndexError):
            ora.run(steps[bad])
        with pytest.raises(MaxSumGpuError, match="no best value"):
            eng.run(steps[bad])


def fuzz_dba(seed, lib_path, steps=STEPS):
    g, p, kw = dba_instance(seed)
    compare_dba_fallible(g, p, kw, lib_path=lib_path, steps=steps)


def fuzz_dpop(seed, lib_path):
    from dpop_common import compare_dpop
    from dpop_oracle import OracleDpop
    g, p, tree, _ = dpop_instance(seed)
    compare_dpop(OracleDpop, g, p, lib_path=lib_path, tree=tree)


# ---- the replica engines: DSA, MGM with keyed draws, MGM-2, R seeded runs in one engine ----------------------
REPLICA_STREAM = 23
REPLICA_COUNTS = (1, 2, 3, 5, 66)        # 66: a second block of the final cost reduction (64 replicas per block)
REPLICA_LARGE = (260, 520)               # variables: the init and the cost launches span blocks
REPLICA_STEPS_LARGE = (0, 1, 3)


def replica_instance(seed):
    """-> (graph, Params, R, {engine: kwargs}, compared replicas, steps).  local_instance; every third seed 260..520
    variables, two replicas compared (the first and the last: the Python oracles dominate) over fewer rounds; else
    every replica up to five, of 66 the two first and the two last (on either side of the second block of 64)."""
    from mgm2_oracle import FAVORS
    large = seed % 3 == 2
    g, _ = local_instance(seed, stream=REPLICA_STREAM, n_vars=REPLICA_LARGE if large else None)
    rng = np.random.default_rng([seed, REPLICA_STREAM, 2])
    p = Params(mode="max" if rng.integers(0, 2) else "min", dtype="f32" if rng.integers(0, 3) == 0 else "f64")
    replicas = int(rng.choice(REPLICA_COUNTS))
    kws = {"dsa": dict(variant="ABC"[int(rng.integers(0, 3))], probability=float(rng.choice([0.3, 0.7, 1.0])),
                       p_mode=["fixed", "arity"][int(rng.integers(0, 2))]),
           "mgm": {},
           "mgm2": dict(favor=FAVORS[int(rng.integers(0, 3))], threshold=float(rng.choice([0.0, 0.3, 0.5, 0.6, 1.0])))}
    if large:
        compared = sorted({0, replicas - 1})
    else:
        compared = list(range(replicas)) if replicas <= 5 else [0, 1, replicas - 2, replicas - 1]
    return g, p, replicas, kws, compared, REPLICA_STEPS_LARGE if large else STEPS


def fuzz_replicas(seed, lib_path):
    """the three replica engines on replica_instance(seed): every compared replica against its single-seed oracle
    bit for bit after every step, all replica costs against tests/replica_cost_reference.py, best() against the
    winner derived from the reference costs (either one where two of them lie within the bound of each other)"""
    from replica_cost_reference import acceptable_winners, check_replica_costs, is_exact
    from replica_shapes_common import ENGINES, same_fields
    g, p, replicas, kws, compared, steps = replica_instance(seed)
    for name in ("dsa", "mgm", "mgm2"):
        E, kw = ENGINES[name], kws[name]
        eng = E["engine"](g, p, kw, seed=seed, seeds=[seed + r for r in range(replicas)], replicas=replicas,
                          lib_path=lib_path)
        oras = {r: E["oracle"](g, p, kw, seed + r) for r in compared}
        done = 0
        for n in steps:
            eng.run(n)
            done += n
            for o in oras.values():
                o.run(n)
            same_fields(E, eng, oras, f"{name} after {done} rounds")
            refs = check_replica_costs(eng, range(replicas))
        if name == "dsa":
            eng.track_best(0)
        b = eng.best()
        w, ok = acceptable_winners([refs[r] for r in range(replicas)], p.mode == "max", is_exact(g, p))
        assert b["replica"] in ok, (name, b["replica"], w, ok)
        assert b["violations"] == refs[b["replica"]][1]
        np.testing.assert_array_equal(b["idx"], refs[b["replica"]][4])
        eng.close()
        for o in oras.values():
            o.close()


def replica_summary(seed):
    """what the oracles alone show of fuzz_replicas(seed): DSA's C oracle for EVERY replica (the Python oracles of
    the other two are too slow for 66 runs), the reference costs of its final states"""
    from oracle.dsa_oracle import OracleDsa
    from replica_cost_reference import CHUNK, acceptable_winners, is_exact, reference_cost
    g, p, replicas, kws, compared, steps = replica_instance(seed)
    starts, finals, refs = [], [], []
    for r in range(replicas):
        o = OracleDsa(g, p, seed=seed + r, **kws["dsa"])
        starts.append(o.assignment()[0].copy())
        o.run(sum(steps))
        finals.append(o.assignment()[0].copy())
        refs.append(reference_cost(g, p, finals[-1]) + (finals[-1],))
        o.close()
    w, ok = acceptable_winners(refs, p.mode == "max", is_exact(g, p))
    return dict(cost_blocks=-(-(g.n_factors + g.n_vars) // CHUNK), replicas=replicas, n_vars=g.n_vars,
                f32_float_tables=p.dtype == "f32" and bool((g.tables != g.tables.astype(np.float32)).any()),
                start_apart=any((s != starts[0]).any() for s in starts), end_apart=any((f != finals[0]).any() for f in finals),
                ambiguous_winner=len(ok) > 1, compared=compared)


# ---- GDBA and DBA as replicas: the recipes of gdba_instance / dba_instance on streams of their own -----------------
# Picked on the oracles alone, as GDBA_STREAM was, over the 48 GPU seeds.  GDBA, of the streams 40..45: 44 gives 5 seeds
# with two or more cost blocks and R > 1 (one of them with 66 replicas), 7 seeds with 66 replicas, replicas that start
# and end apart in 40 of the 40 seeds with R > 1.  DBA, of the streams 40..47: 46 gives 9 seeds with two or more
# violation blocks and R > 1 (3 of them with 66 replicas), 10 seeds with 66 replicas, 11 seeds whose replicas stop in
# different rounds or not at all (7 of them under stop="each"), replicas apart in 40 of 40, and 6 seeds of 48 that end
# early in the "no best value" error (the streams tried gave 6 to 14; the cap is a third of the seeds).
GDBA_REP_STREAM = 44
DBA_REP_STREAM = 46
DBA_STOPS = ("each", "first")            # the stop policy alternates with the seed


def replica_shape(seed, stream):
    """-> (the range of variables or None, R, compared replicas, steps), as replica_instance draws them: every third
    seed REPLICA_LARGE variables, two replicas compared over fewer rounds; R of REPLICA_COUNTS"""
    large = seed % 3 == 2
    replicas = int(np.random.default_rng([seed, stream, 2]).choice(REPLICA_COUNTS))
    if large:
        compared = sorted({0, replicas - 1})
    else:
        compared = list(range(replicas)) if replicas <= 5 else [0, 1, replicas - 2, replicas - 1]
    return REPLICA_LARGE if large else None, replicas, compared, REPLICA_STEPS_LARGE if large else STEPS


def gdba_replica_instance(seed):
    """-> (graph, Params, GDBA kwargs, R, compared replicas, steps): gdba_instance's recipe on GDBA_REP_STREAM"""
    n_vars, replicas, compared, steps = replica_shape(seed, GDBA_REP_STREAM)
    g, p, kw = gdba_instance(seed, stream=GDBA_REP_STREAM, n_vars=n_vars)
    del kw["seed"]
    return g, p, kw, replicas, compared, steps


def dba_replica_instance(seed):
    """-> (graph, Params, DBA kwargs, R, compared replicas, steps, stop policy): dba_instance's recipe on
    DBA_REP_STREAM"""
    n_vars, replicas, compared, steps = replica_shape(seed, DBA_REP_STREAM)
    g, p, kw = dba_instance(seed, stream=DBA_REP_STREAM, pre_stream=(DBA_REP_STREAM, 3), n_vars=n_vars)
    del kw["seed"]
    return g, p, kw, replicas, compared, steps, DBA_STOPS[seed % 2]


def fuzz_gdba_replicas(seed, lib_path):
    """GdbaEngine(replicas=R) on gdba_replica_instance(seed), seeds seed + r: EVERY replica's state against its
    OracleGdba after every step, the stored modifier tables of the compared ones, all device costs against
    tests/replica_cost_reference.py, best() after track_best(0) against the winner derived from the reference costs"""
    from gdba_oracle import OracleGdba
    from gdba_replicas_common import KEYS, n_slots
    from pydcop_amd.gdba import GdbaEngine
    from replica_cost_reference import acceptable_winners, check_replica_costs, is_exact
    g, p, kw, replicas, compared, steps = gdba_replica_instance(seed)
    seeds = [seed + r for r in range(replicas)]
    with GdbaEngine(g, p, seeds=seeds, replicas=replicas, lib_path=lib_path, **kw) as eng:
        oras = [OracleGdba(g, p, seed=s, **kw) for s in seeds]
        done = 0
        for n in steps:
            eng.run(n)
            done += n
            for r, o in enumerate(oras):
                o.run(n)
                se, so = eng.state(r), o.state()
                for k in KEYS:
                    np.testing.assert_array_equal(se[k], so[k], err_msg=f"{k} of replica {r} after {done} rounds")
            for r in compared:
                for s in range(n_slots(g)):
                    np.testing.assert_array_equal(eng.modifiers(s, replica=r), oras[r].modifiers(s),
                                                  err_msg=f"modifiers of slot {s} of replica {r} after {done} rounds")
            refs = check_replica_costs(eng, range(replicas))
        eng.track_best(0)
        b = eng.best()
        w, ok = acceptable_winners([refs[r] for r in range(replicas)], p.mode == "max", is_exact(g, p))
        assert b["replica"] in ok, (b["replica"], w, ok)
        assert b["violations"] == refs[b["replica"]][1]
        np.testing.assert_array_equal(b["idx"], refs[b["replica"]][4])


def dba_replica_oracles(seed):
    """The oracles' side of fuzz_dba_replicas(seed), one round at a time; a generator: after every call of `steps` a row
    dict(rounds, oras, stops, ended, failed) -- the engine's round count after the call, the oracles (one per replica,
    as they are after the call), their stop rounds, the round in which the engine ended (0: it has not), and
    {replica: round} of the oracles that raised IndexError in this call ("no best value"; the last row then).
    stop="each": a replica that stops is frozen, the engine ends once all have stopped.  stop="first": nothing runs
    after the round in which the first replica stops."""
    from dba_oracle import OracleDba
    g, p, kw, replicas, compared, steps, stop = dba_replica_instance(seed)
    oras = [OracleDba(g, p, seed=seed + r, **kw) for r in range(replicas)]
    rounds, ended = 0, 0
    for n in steps:
        failed = {}
        for _ in range(n):
            if ended:
                break
            rounds += 1
            for r, o in enumerate(oras):
                if r in failed:
                    continue
                try:
                    o.run(1)
                except IndexError:
                    failed[r] = rounds
            stops = [o.stop_round for o in oras]
            if not failed and (any(stops) if stop == "first" else all(stops)):
                ended = rounds if stop == "first" else max(stops)
        yield dict(rounds=ended or rounds, oras=oras, stops=[o.stop_round for o in oras], ended=ended, failed=failed)
        if failed:
            break


def dba_failure_names(failed, stop):
    """The replicas the engine's "no best value" error may name: the lowest that has failed by the end of the call.
    stop="each": every replica runs the whole call whatever the others do, so that is the lowest of `failed`.
    stop="first": a replica keeps running after its failure, on a state the reference never has, and may stop there,
    which ends the call for all: the lowest of those that failed up to round j, for any j from the first failure on."""
    if stop == "each":
        return {min(failed)}
    return {min(r for r, k in failed.items() if k <= j) for j in range(min(failed.values()), max(failed.values()) + 1)}


def fuzz_dba_replicas(seed, lib_path):
    """DbaEngine(replicas=R, stop=...) on dba_replica_instance(seed), seeds seed + r, an oracle for EVERY replica: the
    states and weights of the compared ones, the stop rounds, the rounds run, the violations and best() of all after
    every step.  Where an oracle raises IndexError, the engine returns its "no best value" error in the same run
    call, naming the lowest replica that has failed by the end of that call (compare_dba_fallible, per replica);
    everything before that call is compared."""
    import re
    import pytest
    from dba_replicas_common import oracle_violations, ranking, same_state
    from pydcop_amd.dba import DbaEngine
    from pydcop_amd.engine import MaxSumGpuError
    g, p, kw, replicas, compared, steps, stop = dba_replica_instance(seed)
    with DbaEngine(g, p, seeds=[seed + r for r in range(replicas)], replicas=replicas, stop=stop, lib_path=lib_path,
                   **kw) as eng:
        for n, row in zip(steps, dba_replica_oracles(seed)):
            oras = row["oras"]
            if row["failed"]:
                with pytest.raises(MaxSumGpuError, match="no best value") as err:
                    eng.run(n)
                named = int(re.search(r"\(replica (\d+)\)", str(err.value)).group(1))
                assert named in dba_failure_names(row["failed"], stop), (named, row["failed"], stop)
                return
            eng.run(n)
            what = f"after {row['rounds']} rounds ({stop})"
            ran = [row["rounds"] if stop == "first" or not s else s for s in row["stops"]]
            assert [o.cycle_count for o in oras] == ran, what
            ended = row["ended"]
            assert (eng.finished, eng.stop_round, eng.cycle_count) == (bool(ended), ended, row["rounds"]), what
            assert (eng.stop_rounds, eng.rounds_of) == (row["stops"], ran), what
            same_state(eng, {r: oras[r] for r in compared}, what)
            viol = [oracle_violations(o, kw["infinity"]) for o in oras]
            assert list(eng.violations()) == viol, what
            w, b = ranking(viol, row["stops"]), eng.best()
            assert (b["replica"], b["stop_round"], b["violations"]) == (w, row["stops"][w], viol[w]), what
            np.testing.assert_array_equal(b["idx"], oras[w].state()["idx"], err_msg=f"best() {what}")


def gdba_replica_summary(seed):
    """what the oracles alone show of fuzz_gdba_replicas(seed)"""
    from gdba_oracle import OracleGdba
    from replica_cost_reference import CHUNK
    g, p, kw, replicas, compared, steps = gdba_replica_instance(seed)
    starts, finals = [], []
    for r in range(replicas):
        o = OracleGdba(g, p, seed=seed + r, **kw)
        starts.append(o.state()["idx"].copy())
        o.run(sum(steps))
        finals.append(o.state()["idx"].copy())
    return dict(blocks=-(-(g.n_factors + g.n_vars) // CHUNK), replicas=replicas, n_vars=g.n_vars,
                start_apart=any((s != starts[0]).any() for s in starts),
                end_apart=any((f != finals[0]).any() for f in finals))


def dba_replica_summary(seed):
    """what the oracles alone show of fuzz_dba_replicas(seed)"""
    g, p, kw, replicas, compared, steps, stop = dba_replica_instance(seed)
    assert steps[0] == 0
    starts = None
    for last in dba_replica_oracles(seed):
        if starts is None:                  # (the first call runs no round)
            starts = [o.state()["idx"].copy() for o in last["oras"]]
    finals = [o.state()["idx"] for o in last["oras"]]
    return dict(blocks=-(-g.n_factors // 1024), replicas=replicas, n_vars=g.n_vars, stop=stop,
                failed=bool(last["failed"]), mixed_stops=len(set(last["stops"])) > 1, ended=last["ended"],
                start_apart=any((s != starts[0]).any() for s in starts),
                end_apart=any((f != finals[0]).any() for f in finals))


# ---- what the oracles alone show of the sweep (tests/test_fuzz_emu.py asserts that it is not vacuous) ----
def oracle_summary(engine, seed, steps=STEPS):
    from dba_oracle import OracleDba
    from dpop_oracle import OracleDpop
    from gdba_oracle import OracleGdba
    from mgm2_oracle import OracleMgm2
    if engine == "replicas":
        return replica_summary(seed)
    if engine == "gdba_replicas":
        return gdba_replica_summary(seed)
    if engine == "dba_replicas":
        return dba_replica_summary(seed)
    if engine == "dba":
        g, p, kw = dba_instance(seed)
        o, failed = OracleDba(g, p, **kw), False
        try:
            o.run(sum(steps))
        except IndexError:
            failed = True
        return dict(stop_round=o.stop_round, increases=o.increases, moves=o.moves, failed=failed, kw=kw)
    if engine == "gdba":
        g, p, kw = gdba_instance(seed)
        o = OracleGdba(g, p, **kw)
        o.run(sum(steps))
        return dict(pool=int(o.pool[:o.pool_size].sum()), moves=o.moves, kw=kw)
    if engine == "mgm2":
        g, p, kw = mgm2_instance(seed)
        o = OracleMgm2(g, p, **kw)
        o.run(sum(steps))
        return dict(pair_moves=o.pair_moves, kw=kw)
    g, p, tree, shrinks = dpop_instance(seed)
    o = OracleDpop(g, p, tree=tree).solve()
    seps = [dims for dims, _ in o.util.values()]
    return dict(shrinks=shrinks, widest=max([len(d) for d in seps] or [0]),
                one_value_in_separator=any(g.dom_size[u] == 1 for d in seps for u in d),
                entries=o.stats()["total_entries"])


def small_seeds(make, n=5, max_vars=20, ok=lambda *inst: True):
    """the first n seeds whose instance `make(seed)` has at most max_vars variables (the reference is a Python
    message loop) and passes `ok`"""
    out, seed = [], 0
    while len(out) < n:
        inst = make(seed)
        if inst[0].n_vars <= max_vars and ok(*inst):
            out.append(seed)
        seed += 1
    return out


DRIVERS = (fuzz_maxsum, fuzz_others, fuzz_mgm2, fuzz_gdba, fuzz_dba, fuzz_dpop, fuzz_replicas, fuzz_gdba_replicas,
           fuzz_dba_replicas)


if __name__ == "__main__":
    import time
    import dba_common
    from pydcop_amd import engine
    from oracle.maxsum_oracle import build as build_oracles
    build_oracles()
    lib, bad, t0 = dba_common.emu_lib(), 0, time.time()
    engine.register_test_engine(lib)
    for s in range(int(sys.argv[1]), int(sys.argv[2])):
        for f in DRIVERS:
            try:
                f(s, lib)
            except Exception as ex:  # report and go on
                bad += 1
                print("FAIL", f.__name__, "seed", s, repr(ex)[:300], flush=True)
        if s % 25 == 24:
            print("... seed", s, "failures so far:", bad, flush=True)
    print("failures:", bad, f"({time.time() - t0:.0f} s)")
