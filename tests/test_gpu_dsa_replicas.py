"""DSA replicas on the GPU (pydcop_amd/csrc/dsa.hip through the mxs_dsa_* C-ABI 2.7): every replica against the
single-seed oracle bit for bit, the device cost against eval_cost, the best-state records against the oracle-derived
ones.  The tests are those of tests/dsa_replicas_common.py; tests/test_dsa_replicas_emu.py is the CPU twin."""
import pytest

from dsa_replicas_common import (  # noqa: F401  (collected here)
    test_every_replica_equals_the_single_seed_oracle,
    test_many_small_replicas,
    test_explicit_seeds,
    test_replicas_are_distinct_runs,
    test_device_cost_counts_violations_exactly,
    test_best_state_records_equal_the_oracle_derived_ones)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib_path():
    return None
