"""tests/mgm_keyed_oracle.py with `draws="fixed"` against oracle/mgm_oracle.c, bit for bit, on every case and at the
steps the engines are compared on (tests/mgm_common.py): the new oracle's arithmetic is the one already pinned
against the reference (tests/test_mgm_oracle_vs_reference.py); the keyed draws are what it adds."""
import numpy as np
import pytest

from mgm_common import mgm_cases
from mgm_keyed_oracle import OracleMgmKeyed
from pydcop_amd.graph import Params

STEPS = (0, 1, 1, 3, 10, 25)        # compare_mgm's


@pytest.mark.parametrize("case", mgm_cases(), ids=lambda c: c[0])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_fixed_draws_equal_the_c_oracle(case, dtype, oracle_built):
    from oracle.mgm_oracle import OracleMgm
    name, make, kw = case
    g, params = make(), Params(dtype=dtype, **kw)
    new, old = OracleMgmKeyed(g, params, draws="fixed"), OracleMgm(g, params)
    done = 0
    for n in STEPS:
        new.run(n), old.run(n)
        done += n
        assert new.cycle_count == old.cycle_count == done
        sn, so = new.state(), old.state()
        for k in ("idx", "has_cost", "cost", "gain", "new"):
            np.testing.assert_array_equal(sn[k], so[k], err_msg=f"{k} after {done} rounds")
        assert new.eval_cost() == old.eval_cost()
    new.reset(), old.reset()
    new.run(4), old.run(4)
    np.testing.assert_array_equal(new.state()["idx"], old.state()["idx"])
    np.testing.assert_array_equal(new.state()["cost"], old.state()["cost"])
    assert new.late_picks == 0
    old.close()


def test_keyed_draws_change_the_run():
    """the keys matter: another seed, another start; and the generator is the one DSA pins (dsa_uniform)"""
    from oracle.ref_harness import dsa_uniform
    from pydcop_amd import generators as G
    g = G.random_coloring(45, seed=31, variant="hard")
    a, b = OracleMgmKeyed(g, draws="keyed", seed=1), OracleMgmKeyed(g, draws="keyed", seed=2)
    assert (a.cur != b.cur).any()
    v = int(np.flatnonzero(a.has_nb)[0])
    assert a.cur[v] == int(dsa_uniform(1, v, 0, 10) * g.dom_size[v])
    a.run(5)
    again = OracleMgmKeyed(g, draws="keyed", seed=1)
    again.run(2), again.run(3)
    np.testing.assert_array_equal(a.cur, again.cur)
