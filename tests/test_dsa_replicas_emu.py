"""DSA replicas on the emulated engine build (the very same dsa.hip, g++ against the fake HIP runtime): the CPU twin
of tests/test_gpu_dsa_replicas.py.  The tests are those of tests/dsa_replicas_common.py."""
import pytest

from dsa_replicas_common import (  # noqa: F401  (collected here)
    test_every_replica_equals_the_single_seed_oracle,
    test_many_small_replicas,
    test_explicit_seeds,
    test_replicas_are_distinct_runs,
    test_device_cost_counts_violations_exactly,
    test_best_state_records_equal_the_oracle_derived_ones)


@pytest.fixture(scope="module")
def lib_path():
    from emu.build_emu import build
    return build()
