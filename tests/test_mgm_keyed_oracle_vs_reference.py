"""Pins tests/mgm_keyed_oracle.py (`draws="keyed"`) against the REAL reference: the reference's own MgmComputation
objects (pydcop/algorithms/mgm.py) under the keyed generator, run for exactly R rounds by
tests/mgm_keyed_reference.run_reference_mgm_keyed -- selected values and held costs, bit for bit -- and which
engine round a draw of id 11 belongs to: round k (from 1) is made at cycle_count k.  The instances are those of
tests/test_mgm_oracle_vs_reference.py (variable costs on a binary grid: the one order the reference leaves to
PYTHONHASHSEED cannot change a sum).  Where the reference is on the machine."""
import numpy as np
import pytest

from mgm_keyed_oracle import OracleMgmKeyed
from mgm_keyed_reference import run_reference_mgm_keyed
from oracle import ref_harness
from pydcop_amd.graph import Params
from test_mgm_oracle_vs_reference import CASES

pytestmark = pytest.mark.skipif(not ref_harness.reference_available(), reason="reference tree not present")


@pytest.mark.parametrize("name,make,mode", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("rounds", [0, 1, 2, 5, 12])
@pytest.mark.parametrize("seed", [0, 7])
def test_keyed_oracle_equals_reference(name, make, mode, rounds, seed):
    g = make()
    if name == "ising_unaries":   # exact table sums too: k on a binary grid
        g.tables = np.round(g.tables * 64) / 64
    dcop, _ = ref_harness.flat_to_dcop(g, mode)
    index = {n: i for i, n in enumerate(g.var_names)}
    vals, costs, comps, cycles = run_reference_mgm_keyed(dcop, rounds, seed=seed, var_index=index)
    o = OracleMgmKeyed(g, Params(mode=mode), draws="keyed", seed=seed)
    o.run(rounds)
    st = o.state()
    ref_idx = np.array([g.domains[i].index(vals[n]) for i, n in enumerate(g.var_names)])
    np.testing.assert_array_equal(st["idx"], ref_idx)
    for i, n in enumerate(g.var_names):
        if costs[n] is None:
            assert not st["has_cost"][i], n
        else:
            assert st["has_cost"][i] and st["cost"][i] == costs[n], (n, st["cost"][i], costs[n])
    viol, cost = dcop.solution_cost(vals, float("inf"))
    ocost, oviol = o.eval_cost()
    assert oviol == viol and ocost == pytest.approx(cost, rel=1e-12, abs=1e-9)
    # the cycle of the key: the draws of id 11 are made at cycle_count 1 .. rounds, round k at cycle k
    assert set(cycles) <= set(range(1, rounds + 1))
    assert all(c.cycle_count == rounds + 1 for c in comps.values() if c._neighbors) or rounds == 0


def test_the_draws_are_exercised():
    """the hard colouring ties exactly (the comparison leaves out the variable's own cost): some draw of id 11 picks
    beyond the first value, and the start values are not all the first one"""
    name, make, mode = CASES[1]
    o = OracleMgmKeyed(make(), Params(mode=mode), draws="keyed", seed=7)
    assert (o.cur[o.has_nb] > 0).any()
    o.run(12)
    assert o.late_picks > 0
