"""Constructed instances on the edges that random draws hit too rarely, each as small as its edge allows, for
MGM-2, GDBA, DBA and DPOP: `*_edges()` list (name, check), `check(lib_path)` runs the engine and its oracle
through the comparison of tests/{mgm2,gdba,dba,dpop}_common.py (tests/test_fuzz_emu.py on the emulated build,
tests/test_gpu_fuzz.py on the GPU)."""
import numpy as np

from pydcop_amd.graph import Params


def graph_of(dom, scopes, seed, real=True, levels=10, var_cost=None):
    """Constraints over `scopes`, real tables in [-5, 5) or integer ones on `levels` levels"""
    from pydcop_amd.generators import _finish
    rng = np.random.default_rng(seed)
    dom = np.asarray(dom, dtype=np.int32)
    sizes = [int(np.prod(dom[list(sc)])) for sc in scopes]
    tabs = [rng.uniform(-5, 5, n) if real else rng.integers(0, levels, n).astype(np.float64) for n in sizes]
    rowptr = np.zeros(len(scopes) + 1, dtype=np.int32)
    np.cumsum([len(sc) for sc in scopes], out=rowptr[1:])
    toff = np.zeros(len(scopes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=toff[1:])
    vc = rng.uniform(0, 1, int(dom.sum())) if var_cost is None else var_cost
    return _finish(dom, vc, rowptr, np.array([v for sc in scopes for v in sc], dtype=np.int32), np.concatenate(tabs), toff)


# ---- DPOP ----------------------------------------------------------------------------------------------
def _chain(n):
    from pydcop_amd.dpop import pack_tree
    return pack_tree([-1] + list(range(n - 1)), [[v + 1] for v in range(n - 1)] + [[]])


def dpop_hub(as_root):
    """Variable 1, the hub, joins 11 terms, more than the TERM_CACHE = 8 whose offsets the kernel keeps: its own
    costs, then six (seven) child UTILs, then the four (three) constraints it owns.  Below variable 0 the last
    three terms, recomputed for every value, depend on the separator's digit; as the root it is the VALUE step
    alone that walks them."""
    from pydcop_amd.dpop import pack_tree
    dom = [4, 3, 3, 4, 3, 4, 3, 4]
    leaves = list(range(2, 8))
    if as_root:
        scopes = [[v, 1] if v % 2 else [1, v] for v in leaves] + [[0, 1], [1], [1], [1]]
        parent, children = [1, -1] + [1] * 6, [[], leaves + [0]] + [[]] * 6
    else:
        scopes = [[v, 0, 1] if v % 2 else [1, v] for v in leaves] + [[0, 1], [1, 0], [1], [0, 1]]
        parent, children = [-1, 0] + [1] * 6, [[1], leaves] + [[]] * 6
    return graph_of(dom, scopes, 3), pack_tree(parent, children)


def _dpop_check(make, terms=None, utils=None, **pkw):
    def check(lib_path, fuse=None):
        from dpop_common import FUSE, compare_dpop
        from dpop_oracle import OracleDpop
        g, tree = make()
        for dtype in ("f64", "f32"):
            o = compare_dpop(OracleDpop, g, Params(dtype=dtype, **pkw), lib_path=lib_path, tree=tree, fuse=fuse or FUSE)
        if terms:                       # (counted by the oracle: its cost vector, then _terms)
            assert 1 + len(o._terms(terms[0])) == terms[1] > 8
        for v, shape in (utils or {}).items():
            assert o.util[v][1].shape == shape, (v, o.util[v][1].shape)
        return o
    return check


def dpop_edges():
    return [
        ("hub_11_terms", _dpop_check(lambda: dpop_hub(False), terms=(1, 11), utils={1: (4,)})),
        ("hub_11_terms_max", _dpop_check(lambda: dpop_hub(False), terms=(1, 11), mode="max")),
        ("root_11_terms", _dpop_check(lambda: dpop_hub(True), terms=(1, 11))),
        # separators of one-value variables only: UTILs of one entry, no digit at all
        ("separator_of_one_value_variables",
         _dpop_check(lambda: (graph_of([1, 1, 3, 4], [[0, 1, 2], [2, 1], [3, 0], [1, 3], [0, 1]], 4), _chain(4)),
                     utils={1: (1,), 2: (1, 1), 3: (1, 1)})),
        # variable 4 sends a UTIL over (3, 1, 0), variable 1 of one value in the middle; 3 sends one over (1, 0, 2)
        ("one_value_variable_inside_a_separator",
         _dpop_check(lambda: (graph_of([4, 1, 3, 2, 3], [[2, 3], [1, 3], [0, 3], [0, 1, 2], [4, 3], [1, 4, 0]], 5), _chain(5)),
                     utils={4: (2, 1, 4), 3: (1, 4, 3), 2: (1, 4)})),
        # UTILs on the block size and the built-in fuse cap: 128 = 4 * 4 * 8 entries, 129 = 3 * 43
        ("util_128_entries", _dpop_check(lambda: (graph_of([4, 4, 8, 3], [[0, 1, 2, 3], [0, 1], [2]], 6), _chain(4)),
                                         utils={3: (4, 4, 8)})),
        ("util_129_entries", _dpop_check(lambda: (graph_of([3, 43, 2], [[0, 1, 2], [1, 0]], 7), _chain(3)),
                                         utils={2: (3, 43)}, mode="max")),
    ]


# ---- DBA -----------------------------------------------------------------------------------------------
def _violations(g, seed, density, c=1000.0):
    g.tables = c * (np.random.default_rng(seed).random(g.tables.shape[0]) < density)
    g.var_cost = np.zeros_like(g.var_cost)
    return g


def dba_top_domain(top):
    """Twelve variables, the largest domain exactly `top`: run() picks the kernel by it (4 | 5, 8 | 9, 32 | 33)"""
    dom = [top, 2, 3, top - 1, 2, top, 3, 2, top, 3, 2, 3]
    ring = [[i, (i + 1) % 12] if i % 2 else [(i + 1) % 12, i] for i in range(12)]
    scopes = ring + [[0, 5, 1], [3, 8], [6, 2, 9], [8, 4], [10, 0], [7]]
    return _violations(graph_of(dom, scopes, top), top, 0.35)


def dba_slot_counts(dom):
    """One, two and three slots on different variables: the register kernel walks slots in pairs"""
    scopes = [[0, 1], [1, 2], [2, 3], [4, 2], [5, 6], [6, 5, 7], [7, 8], [8, 6], [9, 7]]
    g = _violations(graph_of([dom, dom - 1, dom, dom, 2, 3, dom, 2, dom, 3], scopes, dom), 40 + dom, 0.5)
    assert sorted(set(np.diff(g.var_rowptr))) == [1, 2, 3]
    return g


def dba_idle_wide_variable():
    """A 70-value variable with a unary constraint only never plays: the kernel follows the others' 3 values"""
    scopes = [[i, (i + 1) % 8] for i in range(8)] + [[8], [0, 4], [2, 6, 7]]
    return _violations(graph_of([3] * 8 + [70], scopes, 9), 9, 0.5)


def _dba_check(make, **kw):
    def check(lib_path):
        from dba_common import compare_dba
        from dba_oracle import OracleDba
        compare_dba(OracleDba, make(), Params(), dict(infinity=1000, max_distance=50, seed=11, **kw), lib_path=lib_path)
    return check


def dba_edges():
    return ([(f"top_domain_{d}", _dba_check(lambda d=d: dba_top_domain(d))) for d in (4, 5, 8, 9, 32, 33)]
            + [(f"slot_counts_dom{d}", _dba_check(lambda d=d: dba_slot_counts(d))) for d in (4, 8, 32, 40)]
            + [("idle_wide_variable", _dba_check(dba_idle_wide_variable))])


# ---- MGM-2 ---------------------------------------------------------------------------------------------
def offer_entries(g):
    """the entries of all offer tables: per variable (own values) x (the largest neighbour domain)"""
    scopes = [set(int(u) for u in g.edge_var[g.factor_rowptr[f]:g.factor_rowptr[f + 1]]) for f in range(g.n_factors)]
    total = 0
    for v in range(g.n_vars):
        nb = set().union(*[s for s in scopes if v in s] or [set()]) - {v}
        total += int(g.dom_size[v]) * max([int(g.dom_size[u]) for u in nb] or [0])
    return total


def mgm2_unequal_partners():
    """Pairs of a 2-value and a 9-value variable (either may offer: rows of 9 and rows of 2), and stars whose
    centre has neighbours of 9 and of 3 values: its offer rows are 9 wide, a partner of 3 values fills 3."""
    dom, scopes = [], []
    for i in range(12):
        a = len(dom)
        dom += [2, 9] if i % 2 else [9, 2]
        scopes += [[a, a + 1]] + ([[a + 1, a]] if i % 3 == 0 else [])
    for centre in (2, 9, 3):
        a = len(dom)
        dom += [centre, 9, 3, 2]
        scopes += [[a, a + 1], [a + 2, a], [a, a + 3]]
    return graph_of(dom, scopes, 12, real=False)


def mgm2_entries(total):
    """Offer tables of exactly 256 / 257 entries in all: the edge of one block of the offer-entry launch"""
    if total == 256:
        dom, scopes = [8, 8, 4, 8, 4, 4, 4, 4], [[0, 1], [2, 3], [4, 5], [7, 6]]
    else:       # a path over domains (1, 3, 2) holds 3 + 6 + 6 = 15 entries
        dom, scopes = [8, 8, 4, 8, 5, 5, 1, 3, 2], [[0, 1], [2, 3], [5, 4], [6, 7], [7, 8]]
    g = graph_of(dom, scopes, total, real=False)
    assert offer_entries(g) == total
    return g


def _mgm2_check(make, **kw):
    def check(lib_path):
        from mgm2_common import compare_mgm2
        from mgm2_oracle import OracleMgm2
        for mode in ("min", "max"):
            compare_mgm2(OracleMgm2, make(), Params(mode=mode), dict(seed=13, **kw), lib_path=lib_path)
    return check


def mgm2_edges():
    return ([(f"unequal_partners_{f}", _mgm2_check(mgm2_unequal_partners, favor=f, threshold=0.5))
             for f in ("unilateral", "no", "coordinated")]
            + [(f"offer_entries_{n}", _mgm2_check(lambda n=n: mgm2_entries(n), threshold=0.6)) for n in (256, 257)])


# ---- GDBA ----------------------------------------------------------------------------------------------
def gdba_live_130():
    """130 variables (three blocks of 64 threads, the last with two) on disjoint triples of domains (2, 5, 3)
    under one or two arity-3 constraints, pairs, stars and paths: every slot of a triple, a pair and a leaf is
    live in modes E, R and C.  Real tables."""
    dom, scopes = [], []
    for i in range(30):
        a = len(dom)
        dom += [2, 5, 3]
        scopes += [[a, a + 1, a + 2]] + ([[a + 2, a, a + 1]] if i % 3 == 0 else [])
    for i in range(10):
        a = len(dom)
        dom += [5, 2] if i % 2 else [3, 5]
        scopes += [[a, a + 1]] + ([[a + 1, a]] if i % 4 == 0 else [])
    for leaves in (4, 4):
        a = len(dom)
        dom += [3] + [2, 5, 3, 2][:leaves]
        scopes += [[a, a + 1 + i] if i % 2 else [a + 1 + i, a] for i in range(leaves)]
    for _ in range(2):
        a = len(dom)
        dom += [2, 5, 3, 5, 2]
        scopes += [[a + i, a + i + 1] for i in range(4)]
    assert len(dom) == 130
    order = np.random.default_rng(14).permutation(len(scopes))
    return graph_of(dom, [scopes[i] for i in order], 14, var_cost=np.zeros(int(np.sum(dom))))


def _gdba_check(vio, inc):
    def check(lib_path):
        from gdba_common import compare_gdba
        from gdba_oracle import OracleGdba
        kw = dict(modifier="M", violation=vio, increase_mode=inc, seed=15)
        for mode in ("min", "max"):
            compare_gdba(OracleGdba, gdba_live_130(), Params(mode=mode, dtype="f32"), kw, lib_path=lib_path)
    return check


def gdba_edges():
    return [(f"live_130_M_{vio}_{inc}_f32", _gdba_check(vio, inc)) for inc in ("R", "C") for vio in ("NZ", "NM", "MX")]


def all_edges():
    return [(f"{algo}_{name}", check) for algo, edges in (("dpop", dpop_edges()), ("dba", dba_edges()), ("mgm2", mgm2_edges()),
                                                         ("gdba", gdba_edges())) for name, check in edges]
