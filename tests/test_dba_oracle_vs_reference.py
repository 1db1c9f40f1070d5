"""Pins tests/dba_oracle.py against the REAL reference: the reference's own DbaComputation objects
(pydcop/algorithms/dba.py) run under keyed draws by tests/dba_reference.run_reference_dba -- values, held
costs, evals, improvements, new values, termination counters, consistent flags, every weight, the stop
round and the number of moves.  Where the reference is on the machine (oracle/stage_reference.locate())."""
import numpy as np
import pytest

from oracle import ref_harness

pytestmark = pytest.mark.skipif(not ref_harness.reference_available(), reason="reference tree not present")


def check_against_reference(g, kw, rounds):
    from dba_common import STATE_KEYS
    from dba_oracle import OracleDba
    from dba_reference import reference_state
    from pydcop_amd.graph import Params
    ref, weights, info = reference_state(g, kw, rounds)
    o = OracleDba(g, Params(), **kw)
    o.run(rounds)
    st = o.state()
    for key in STATE_KEYS:
        np.testing.assert_array_equal(st[key], ref[key], err_msg=key)
    np.testing.assert_array_equal(o.weights(), weights)
    assert (o.cycle_count, o.stop_round, o.moves) == (info["rounds"], info["stop_round"], info["moves"])
    return info, int((weights - 1).sum())


@pytest.mark.parametrize("case", __import__("dba_common").dba_cases(), ids=lambda c: c[0])
def test_dba_oracle_equals_reference(case):
    from dba_common import ROUNDS
    name, make, kw = case
    info, _ = check_against_reference(make(), kw, ROUNDS)
    assert info["moves"] > 0, "nothing moved: the case proves nothing"


@pytest.mark.parametrize("rounds", [0, 1, 2, 5])
@pytest.mark.parametrize("pick", [0, 3, 7, 9])
def test_dba_oracle_equals_reference_early_rounds(pick, rounds):
    from dba_common import dba_cases
    name, make, kw = dba_cases()[pick]
    check_against_reference(make(), kw, rounds)


def test_dba_reference_raises_where_infinity_is_too_small():
    """`infinity: 1`: weights start at 1, so every violation already reaches infinity -- the reference raises
    IndexError (random.choice of an empty list), and so does the oracle."""
    from dba_common import scaled
    from dba_oracle import OracleDba
    from dba_reference import reference_state
    from mgm_common import repeated_pairs_and_unaries
    from pydcop_amd.graph import Params
    g = scaled(repeated_pairs_and_unaries(30, 87))
    kw = dict(infinity=1, max_distance=50, seed=7)
    with pytest.raises(IndexError):
        reference_state(g, kw, 3)
    with pytest.raises(IndexError):
        OracleDba(g, Params(), **kw).run(3)


def test_dba_reference_refuses_max():
    from dba_oracle import OracleDba
    from oracle.ref_harness import flat_to_dcop
    from dba_reference import run_reference_dba
    from pydcop_amd import generators as G
    from pydcop_amd.graph import Params
    g = G.random_coloring(10, seed=1, variant="hard", unary_noise=0)
    dcop, _ = flat_to_dcop(g, "max")
    with pytest.raises(ValueError, match="satisfaction"):
        run_reference_dba(dcop, 1)
    with pytest.raises(ValueError, match="satisfaction"):
        OracleDba(g, Params(mode="max"))


def _fuzz_seeds():
    from fuzz_common import dba_instance, small_seeds
    return small_seeds(dba_instance, n=6)


@pytest.mark.parametrize("seed", _fuzz_seeds())
def test_dba_oracle_equals_reference_on_random_instances(seed):
    """the small end of the sweep of tests/fuzz_common.py: domains up to 65 values, `infinity` of 1000, 999.5
    and 2 (an eval can equal it); where the oracle raises IndexError, so does the reference"""
    from dba_oracle import OracleDba
    from dba_reference import reference_state
    from fuzz_common import STEPS, dba_failing_step, dba_instance
    from pydcop_amd.graph import Params
    g, p, kw = dba_instance(seed)
    rounds = (1, 4, 10)
    bad = dba_failing_step(g, p, kw, rounds)
    for n in rounds[:bad]:
        check_against_reference(g, kw, n)
    if bad is not None:
        with pytest.raises(IndexError):
            reference_state(g, kw, rounds[bad])
