"""MGM-2 replicas on the GPU (pydcop_amd/csrc/mgm2.h through mxs_mgm2_create_replicas): every replica against the
oracle bit for bit, the device cost against eval_cost, the best replica against the oracle-derived winner, the fixtures
recorded from the reference.  The tests are those of tests/mgm2_replicas_common.py; tests/test_mgm2_replicas_emu.py is
the CPU twin."""
import pytest

from mgm2_replicas_common import (  # noqa: F401  (collected here)
    test_every_replica_equals_the_oracle,
    test_many_small_replicas,
    test_explicit_seeds,
    test_one_replica_equals_the_single_run_engine,
    test_refusals,
    test_reference_fixtures,
    test_fixture_set_is_complete,
    test_device_costs_and_the_best_replica)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib_path():
    return None
