"""GDBA replicas on the emulated engine build (the very same gdba.h, g++ against the fake HIP runtime): the CPU twin
of tests/test_gpu_gdba_replicas.py.  The tests are those of tests/gdba_replicas_common.py."""
import pytest

from gdba_replicas_common import (  # noqa: F401  (collected here)
    test_every_replica_equals_the_oracle,
    test_many_small_replicas,
    test_explicit_seeds,
    test_one_replica_equals_the_single_run_engine,
    test_reference_fixtures,
    test_fixture_set_is_complete,
    test_best_state_records_equal_the_oracle_derived_ones,
    test_gdba_best_state_snapshots_span_blocks,
    test_device_costs_in_max_mode_with_float_tables,
    test_refusals)


@pytest.fixture(scope="module")
def lib_path():
    from emu.build_emu import build
    return build()
