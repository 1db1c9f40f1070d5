"""GDBA: the cases and the engine-vs-oracle comparison shared by the emulated (CPU) and the GPU tests."""
import itertools

import numpy as np

from mgm_common import repeated_pairs_and_unaries, shuffled_names, with_init
from pydcop_amd import generators as G
from pydcop_amd.gdba import GdbaEngine

ROUNDS = 12


def from_scopes(dom_size, scopes, rng, lo=0, hi=10, var_cost=None):
    """Integer tables `integers(lo, hi)` over the given scopes."""
    from pydcop_amd.generators import _finish
    dom_size = np.asarray(dom_size, dtype=np.int32)
    tabs = [rng.integers(lo, hi, size=int(np.prod(dom_size[list(sc)]))).astype(np.float64) for sc in scopes]
    rowptr = np.zeros(len(scopes) + 1, dtype=np.int32)
    np.cumsum([len(sc) for sc in scopes], out=rowptr[1:])
    toff = np.zeros(len(scopes) + 1, dtype=np.int64)
    np.cumsum([t.size for t in tabs], out=toff[1:])
    vc = np.zeros(int(dom_size.sum())) if var_cost is None else var_cost
    return _finish(dom_size, vc, rowptr, np.array([v for sc in scopes for v in sc], dtype=np.int32),
                   np.concatenate(tabs), toff)


def dyadic_var_costs(g, seed):
    """Variable costs k / 64: their sums are exact in any order (tests/gdba_oracle.py, Determinism)."""
    g.var_cost = np.random.default_rng(seed).integers(0, 8, g.var_cost.shape[0]) / 64.0
    return g


def stars_paths_unaries(seed):
    """Stars and paths (a leaf's single constraint covers all its neighbours: live modifier tables), unary
    constraints on some of them, a variable without neighbours, dyadic variable costs."""
    rng = np.random.default_rng(seed)
    scopes, n = [], 0
    for leaves in (3, 4, 2):                                   # stars: centre n, leaves after it
        scopes += [[n, n + 1 + i] if i % 2 else [n + 1 + i, n] for i in range(leaves)]
        n += leaves + 1
    for length in (2, 3, 5, 2, 4):                             # paths
        scopes += [[n + i, n + i + 1] for i in range(length - 1)]
        n += length
    n += 1                                                     # one variable with a unary constraint only
    scopes += [[int(v)] for v in rng.choice(n, size=n // 3, replace=False)] + [[n - 1]]
    order = rng.permutation(len(scopes))
    g = from_scopes(np.full(n, 3), [scopes[i] for i in order], rng, 0, 4)
    return dyadic_var_costs(g, seed)


def triples_arity3(seed):
    """Arity-3 constraints over mixed domains: disjoint triples (every slot live), two triples sharing a
    variable (dead slots for it), and a pair of constraints over the same triple."""
    rng = np.random.default_rng(seed)
    dom = rng.choice([2, 3, 4], size=24)
    scopes = [[3 * i, 3 * i + 1, 3 * i + 2] for i in range(8)]
    scopes += [[2, 3, 7], [10, 9, 11], [12, 13], [16]]
    order = rng.permutation(len(scopes))
    return with_init(from_scopes(dom, [scopes[i] for i in order], rng, 0, 3), seed)


def matched_pairs_binary(seed):
    """Disjoint pairs with two or three 0 / 1 constraints each, in both orientations (every slot live, conflicts
    that no move resolves), shuffled names."""
    rng = np.random.default_rng(seed)
    scopes = []
    for i in range(14):
        a, b = 2 * i, 2 * i + 1
        scopes += [[a, b], [b, a]] + ([[a, b]] if i % 3 == 0 else [])
    order = rng.permutation(len(scopes))
    return shuffled_names(from_scopes(np.full(28, 3), [scopes[i] for i in order], rng, 0, 2), seed)


# instances with live slots for E, R and C (leaves, disjoint scopes) ...
LIVE = [
    ("soft_deg2", lambda: G.random_coloring(30, avg_degree=2, seed=81, unary_noise=0)),
    ("hard_deg2_shuffled", lambda: shuffled_names(G.random_coloring(30, avg_degree=2, seed=82, variant="hard",
                                                                    unary_noise=0), 82)),
    ("matched_pairs_binary", lambda: matched_pairs_binary(92)),
    ("stars_paths_unaries", lambda: stars_paths_unaries(83)),
    ("triples_arity3_init", lambda: triples_arity3(84)),
]
# ... and the general ones (mode T is live everywhere)
GENERAL = [
    ("soft_deg4", lambda: G.random_coloring(30, seed=85, unary_noise=0)),
    ("hard_deg4_init", lambda: with_init(G.random_coloring(30, seed=86, variant="hard", unary_noise=0), 86)),
    ("repeated_pairs_unaries", lambda: dyadic_var_costs(repeated_pairs_and_unaries(30, 87), 87)),
    ("mixed_int_arity3", lambda: G.random_mixed(24, 36, seed=88, float_tables=False, unary_noise=0)),
]


def gdba_cases():
    """(name, graph factory, Params kwargs, GDBA kwargs): the 24 variants, each in min and in max."""
    cases = []
    combos = itertools.product(("A", "M"), ("NZ", "NM", "MX"), ("E", "R", "C", "T"), ("min", "max"))
    for i, (mod, vio, inc, mode) in enumerate(combos):
        # an instance on which the variant both moves and increases within ROUNDS rounds: in min mode a leaf of a
        # hard colouring is never stuck on a violated constraint, MX needs tables whose maximum no move avoids,
        # and in max mode (moves go to the LEAST improving variable of a neighbourhood) the soft instances stall
        k = i // 2 + i // 8
        if inc == "T":
            pick = (1, 2)[k % 2] if mode == "max" else k % 4
            iname, make = GENERAL[pick]
        else:
            pick = (1, 3)[k % 2] if mode == "max" else (2 if vio == "MX" else (0, 2, 3, 4)[k % 4])
            iname, make = LIVE[pick]
        cases.append((f"{mod}_{vio}_{inc}_{mode}_{iname}", make, {"mode": mode},
                      dict(modifier=mod, violation=vio, increase_mode=inc, seed=i + 1)))
    # float tables: the sums in the reference's order matter bit for bit
    cases.append(("A_NM_T_min_mixed_float", lambda: G.random_mixed(24, 36, seed=89, unary_noise=0), {"mode": "min"},
                  dict(modifier="A", violation="NM", increase_mode="T", seed=90)))
    cases.append(("M_NM_E_min_float_deg2", lambda: _float_tables(G.random_coloring(30, avg_degree=2, seed=91, unary_noise=0)),
                  {"mode": "min"}, dict(modifier="M", violation="NM", increase_mode="E", seed=91)))
    return cases


def _float_tables(g):
    g.tables = np.random.default_rng(5).uniform(0.0, 2.0, g.tables.shape[0])
    return g


def same_state(eng, ora, what=""):
    se, so = eng.state(), ora.state()
    for key in ("idx", "has_cost", "cost", "improve", "new"):
        np.testing.assert_array_equal(se[key], so[key], err_msg=f"{key} {what}")


def same_modifiers(eng, ora, what=""):
    for s in range(len(ora.graph.var_edges)):
        np.testing.assert_array_equal(eng.modifiers(s), ora.modifiers(s), err_msg=f"modifiers of slot {s} {what}")


def compare_gdba(oracle_cls, graph, params, kw, lib_path=None, steps=(0, 1, 1, 3, 7)):
    """Round-by-round state (values, held costs, improvements, new values) and every stored modifier table, bit
    for bit; 1 + 1 + 3 rounds are the state after 5; reset starts again."""
    eng = GdbaEngine(graph, params, lib_path=lib_path, **kw)
    ora = oracle_cls(graph, params, **kw)
    done = 0
    for n in steps:
        eng.run(n), ora.run(n)
        done += n
        assert eng.cycle_count == ora.cycle_count == done
        same_state(eng, ora, f"after {done} rounds")
        same_modifiers(eng, ora, f"after {done} rounds")
        ce, co = eng.eval_cost(), ora.eval_cost()
        assert ce[1] == co[1] and abs(ce[0] - co[0]) <= 1e-9 * max(1.0, abs(co[0]))
    after5 = None
    eng.reset(), ora.reset()
    assert eng.cycle_count == 0
    same_state(eng, ora, "after reset")
    same_modifiers(eng, ora, "after reset")
    eng.run(5), ora.run(5)
    after5 = eng.state()
    same_state(eng, ora, "5 rounds after reset")
    same_modifiers(eng, ora, "5 rounds after reset")
    eng.reset()
    for n in (1, 1, 3):
        eng.run(n)
    for key, val in eng.state().items():
        np.testing.assert_array_equal(val, after5[key], err_msg=f"{key}: 1 + 1 + 3 rounds against 5")
    eng.close(), ora.close()


def gdba_golden_files():
    import glob
    import os
    return sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gdba", "*.npz")))


def load_gdba_golden(path):
    """tools/make_golden_gdba.py -> (FlatGraph, Params kwargs, GDBA kwargs, rounds, ref): ref holds what the
    reference's own computations held after `rounds` rounds -- idx, cost (NaN: still None), improve, new and
    the modifier tables of the stored slots (mod_off[s] .. mod_off[s + 1] of mod)."""
    import json
    from pydcop_amd.graph import FlatGraph
    z = np.load(path)
    meta = json.loads(bytes(z["meta"]).decode())
    g = FlatGraph(dom_size=z["dom_size"], var_cost=z["var_cost"], factor_rowptr=z["factor_rowptr"],
                  edge_var=z["edge_var"], table_off=z["table_off"], tables=z["tables"],
                  var_rowptr=z["var_rowptr"], var_edges=z["var_edges"],
                  init_idx=z["init_idx"] if "init_idx" in z.files else None)
    g.var_names = meta["var_names"]
    ref = {k: z["ref_" + k] for k in ("idx", "cost", "improve", "new", "mod", "mod_off")}
    return g.validate(), {"mode": meta["mode"]}, meta["gdba"], meta["rounds"], ref


def check_golden(eng, ref):
    """`eng`: a GdbaEngine or the oracle, after the fixture's rounds"""
    state = eng.state()
    np.testing.assert_array_equal(state["idx"], ref["idx"])
    held = ~np.isnan(ref["cost"])
    np.testing.assert_array_equal(state["has_cost"].astype(bool), held)
    np.testing.assert_array_equal(state["cost"][held], ref["cost"][held])
    np.testing.assert_array_equal(state["improve"], ref["improve"])
    np.testing.assert_array_equal(state["new"], ref["new"])
    off = ref["mod_off"]
    for s in range(len(off) - 1):
        np.testing.assert_array_equal(eng.modifiers(s), ref["mod"][off[s]:off[s + 1]], err_msg=f"slot {s}")
