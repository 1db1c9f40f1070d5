"""MGM with keyed draws and replicas on the emulated engine build (the very same mgm.hip, g++ against the fake HIP
runtime): the CPU twin of tests/test_gpu_mgm_replicas.py.  The tests are those of tests/mgm_replicas_common.py."""
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


@pytest.fixture(scope="module")
def lib_path():
    from emu.build_emu import build
    return build()
