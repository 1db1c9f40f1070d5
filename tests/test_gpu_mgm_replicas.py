"""MGM with keyed draws and replicas on the GPU (pydcop_amd/csrc/mgm.hip through mxs_mgm_create_keyed): every replica
against the keyed oracle bit for bit, the device cost against eval_cost, the best replica against the oracle-derived
winner, the fixtures recorded from the reference.  The tests are those of tests/mgm_replicas_common.py;
tests/test_mgm_replicas_emu.py is the CPU twin."""
import pytest

from mgm_replicas_common import (  # noqa: F401  (collected here)
    test_every_replica_equals_the_keyed_oracle,
    test_many_small_replicas,
    test_explicit_seeds,
    test_device_costs_and_the_best_replica,
    test_keyed_single_run_differs_from_the_fixed_draws,
    test_fixed_draws_still_equal_the_c_oracle,
    test_reference_fixtures,
    test_fixture_set_is_complete)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib_path():
    return None
