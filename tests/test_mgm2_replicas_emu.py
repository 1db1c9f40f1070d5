"""MGM-2 replicas on the emulated engine build (the very same mgm2.h, g++ against the fake HIP runtime): the CPU twin
of tests/test_gpu_mgm2_replicas.py.  The tests are those of tests/mgm2_replicas_common.py."""
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


@pytest.fixture(scope="module")
def lib_path():
    from emu.build_emu import build
    return build()
