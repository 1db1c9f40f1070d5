"""tests/replica_cost_reference.py against two other statements of the same sum: exact rational arithmetic over the
instance written out constraint by constraint, and -- where the reference is on the machine -- the reference's own
DCOP.solution_cost (pydcop/dcop/dcop.py:308-367).  No engine build is loaded."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import ref_harness
from pydcop_amd import generators as G
from pydcop_amd.graph import Params
from replica_cost_reference import (INF, U, assert_chunks_carry_weight, assert_chunks_hold_violations, cost_bound,
                                    is_exact, reference_cost, reference_items)


def with_eval_costs(g, seed):
    g.eval_var_cost = np.random.default_rng(seed).uniform(-1.0, 1.0, size=g.var_cost.shape[0])
    return g


def rational_cost(g, dtype, idx, infinity):
    """the same cost from per-constraint numpy views (reshape and index, no row-major arithmetic), summed exactly"""
    total, hard, n = Fraction(0), 0, 0
    for f in range(g.n_factors):
        scope = g.edge_var[g.factor_rowptr[f]:g.factor_rowptr[f + 1]]
        table = g.tables[g.table_off[f]:g.table_off[f + 1]].reshape([int(g.dom_size[v]) for v in scope])
        e = table[tuple(int(idx[v]) for v in scope)]
        e = float(np.float32(e)) if dtype == "f32" else float(e)
        n += 1
        if e == infinity:
            hard += 1
        else:
            total += Fraction(e)
    own = g.eval_var_cost if g.eval_var_cost is not None else g.var_cost
    for v in range(g.n_vars):
        e = float(own[int(g.cost_off[v]) + int(idx[v])])
        n += 1
        if e == infinity:
            hard += 1
        else:
            total += Fraction(e)
    return total, hard, n


CASES = [
    ("mixed_f64", lambda: G.random_mixed(30, 65, seed=34, dom_choices=(2, 3, 4)), "f64", INF),
    ("mixed_f32", lambda: G.random_mixed(30, 65, seed=34, dom_choices=(2, 3, 4)), "f32", INF),
    ("hard", lambda: G.random_coloring(45, seed=31, variant="hard"), "f64", 1000.0),
    ("hard_f32_eval_costs", lambda: with_eval_costs(G.random_coloring(45, seed=31, variant="hard"), 3), "f32", 1000.0),
    ("arity4", lambda: G.random_mixed(12, 30, seed=5, max_arity=4, dom_choices=(1, 2, 5)), "f64", INF),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_reference_cost_equals_the_exact_rational_sum(case):
    name, make, dtype, infinity = case
    g, rng = make(), np.random.default_rng(7)
    for _ in range(4):
        idx = rng.integers(0, g.dom_size)
        cost, viol, sum_abs, items = reference_cost(g, Params(dtype=dtype), idx, infinity)
        total, hard, n = rational_cost(g, dtype, idx, infinity)
        assert (viol, items) == (hard, n) and items == g.n_factors + g.n_vars
        assert cost == float(total)         # both are the exact sum rounded once
        assert sum_abs >= abs(cost)
        if name.startswith("hard"):
            assert viol > 0
    if name == "mixed_f32":     # the narrowing is seen: these tables are not f32-exact
        assert reference_cost(g, Params(dtype="f32"), idx)[0] != reference_cost(g, Params(), idx)[0]


def test_eval_var_cost_replaces_var_cost():
    g = G.random_coloring(20, seed=1)
    idx = np.zeros(20, dtype=np.int32)
    plain = reference_items(g, Params(), idx)
    g.eval_var_cost = g.var_cost + 1.0
    assert reference_items(g, Params(), idx)[g.n_factors:] == [x + 1.0 for x in plain[g.n_factors:]]
    assert reference_items(g, Params(), idx)[:g.n_factors] == plain[:g.n_factors]


def test_the_bound_and_the_exact_cases():
    assert cost_bound(1, 5.0) == 0.0 and cost_bound(0, 0.0) == 0.0
    assert cost_bound(1025, 1.0) == 1024 * U / (1 - 1024 * U)
    assert is_exact(G.random_coloring(20, seed=1, variant="hard", unary_noise=0), Params())
    assert not is_exact(G.random_coloring(20, seed=1, variant="hard"), Params())            # variable costs
    assert not is_exact(G.random_mixed(20, 30, seed=1, unary_noise=0), Params())            # real-valued tables
    # a sum in another order stays inside the bound, a dropped item does not
    g = G.random_mixed(300, 800, seed=34, dom_choices=(2, 3, 4))
    idx = np.random.default_rng(1).integers(0, g.dom_size)
    items = reference_items(g, Params(), idx)
    cost, _, sum_abs, n = reference_cost(g, Params(), idx)
    back = 0.0
    for x in reversed(items):
        back += x
    assert abs(back - cost) <= cost_bound(n, sum_abs) < 1e-9
    assert abs(math.fsum(items[:-1]) - cost) > cost_bound(n, sum_abs)


def test_the_non_vacuity_conditions_can_fail():
    g = G.random_mixed(300, 800, seed=34, dom_choices=(2, 3, 4))
    idx = np.random.default_rng(1).integers(0, g.dom_size)
    assert_chunks_carry_weight(g, Params(), idx)
    g.tables[:] = 0.0
    with pytest.raises(AssertionError, match="sum to"):
        assert_chunks_carry_weight(g, Params(), idx)
    h = G.random_coloring(700, seed=32, variant="hard", unary_noise=0)
    assert_chunks_hold_violations(h, Params(), np.zeros(700, dtype=np.int32), 1000.0)       # one colour: all violated
    h.tables[:] = 0.0
    with pytest.raises(AssertionError, match="no violation"):
        assert_chunks_hold_violations(h, Params(), np.zeros(700, dtype=np.int32), 1000.0)


@pytest.mark.skipif(not ref_harness.reference_available(), reason="reference tree not present")
@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("mixed_f64", "hard", "arity4")], ids=lambda c: c[0])
def test_reference_cost_equals_the_reference_projects_solution_cost(case):
    name, make, dtype, infinity = case
    g = make()
    dcop, _ = ref_harness.flat_to_dcop(g, "min")
    rng = np.random.default_rng(11)
    for _ in range(3):
        idx = rng.integers(0, g.dom_size)
        vals = {n: g.domains[i][int(idx[i])] for i, n in enumerate(g.var_names)}
        viol, cost = dcop.solution_cost(vals, infinity)
        ref = reference_cost(g, Params(), idx, infinity)
        assert viol == ref[1]
        assert abs(cost - ref[0]) <= cost_bound(ref[3], ref[2])
