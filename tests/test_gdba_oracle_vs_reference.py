"""Pins tests/gdba_oracle.py against the REAL reference: the reference's own GdbaComputation objects
(pydcop/algorithms/gdba.py) run for exactly R rounds under keyed draws by
tests/gdba_reference.run_reference_gdba -- values, held costs, improvements, new values and every
modifier entry a look-up can reach, bit for bit; the entries of the slots the oracle does not store
(dead in E, R, C) are checked to be still at their base in the reference.  Where the reference is on
the machine (oracle/stage_reference.locate())."""
import numpy as np
import pytest

from oracle import ref_harness

pytestmark = pytest.mark.skipif(not ref_harness.reference_available(), reason="reference tree not present")


def check_against_reference(g, mode, kw, rounds):
    from gdba_oracle import OracleGdba
    from gdba_reference import reference_state
    from pydcop_amd.graph import Params
    ref, mods, moves, (cost, viol) = reference_state(g, mode, kw, rounds)
    o = OracleGdba(g, Params(mode=mode), **kw)
    o.run(rounds)
    st = o.state()
    np.testing.assert_array_equal(st["idx"], ref["idx"])
    held = ~np.isnan(ref["cost"])
    np.testing.assert_array_equal(st["has_cost"].astype(bool), held)
    np.testing.assert_array_equal(st["cost"][held], ref["cost"][held])
    np.testing.assert_array_equal(st["improve"], ref["improve"])
    np.testing.assert_array_equal(st["new"], ref["new"])
    assert o.moves == moves
    base = 0 if kw["modifier"] == "A" else 1
    non_base = 0
    for s, m in enumerate(mods):
        mine = o.modifiers(s)
        if len(mine) == 0:                      # not stored: no look-up of the reference ever sees an increase
            assert (m == base).all(), s
        elif kw["increase_mode"] == "T":
            assert (m == mine[0]).all(), s
            non_base += int(mine[0] != base)
        else:
            np.testing.assert_array_equal(mine, m, err_msg=f"slot {s}")
            non_base += int((m != base).sum())
    ocost, oviol = o.eval_cost()
    assert oviol == viol and ocost == pytest.approx(cost, rel=1e-12, abs=1e-9)
    return moves, non_base


@pytest.mark.parametrize("case", __import__("gdba_common").gdba_cases(), ids=lambda c: c[0])
def test_gdba_oracle_equals_reference(case):
    from gdba_common import ROUNDS
    name, make, pkw, kw = case
    moves, non_base = check_against_reference(make(), pkw["mode"], kw, ROUNDS)
    assert moves > 0, "nothing moved: the case proves nothing"
    assert non_base > 0, "no modifier left its base: the case proves nothing"


@pytest.mark.parametrize("rounds", [0, 1, 2, 5])
@pytest.mark.parametrize("pick", [0, 13, 26, 39])
def test_gdba_oracle_equals_reference_early_rounds(pick, rounds):
    from gdba_common import gdba_cases
    name, make, pkw, kw = gdba_cases()[pick]
    check_against_reference(make(), pkw["mode"], kw, rounds)


def _fuzz_seeds():
    from fuzz_common import gdba_instance, small_seeds
    from pydcop_amd.dpop import neighbor_lists

    def ok(g, p, kw):
        # real-valued variable costs: the reference sums them in the order of a Python set (gdba_oracle.py);
        # mode C walks every assignment of a variable's neighbours in Python
        walk = max(int(np.prod(g.dom_size[nb], dtype=np.int64)) for nb in neighbor_lists(g))
        return bool((g.var_cost * 64 == np.round(g.var_cost * 64)).all()) and walk <= 500
    return small_seeds(gdba_instance, ok=ok)


@pytest.mark.parametrize("seed", _fuzz_seeds())
def test_gdba_oracle_equals_reference_on_random_instances(seed):
    """the small end of the sweep of tests/fuzz_common.py: unequal domains, arities up to 4, the seed's variant"""
    from fuzz_common import gdba_instance
    g, p, kw = gdba_instance(seed)
    for rounds in (1, 4, 10):
        check_against_reference(g, p.mode, kw, rounds)
