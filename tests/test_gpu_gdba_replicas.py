"""GDBA replicas on the GPU (pydcop_amd/csrc/gdba.h through mxs_gdba_create_replicas): every replica against the
oracle bit for bit, modifier tables included, the device cost against eval_cost, the best-state records against the
oracle-derived ones, the fixtures recorded from the reference.  The tests are those of tests/gdba_replicas_common.py;
tests/test_gdba_replicas_emu.py is the CPU twin."""
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

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib_path():
    return None


def test_gdba_replica_symbols_are_exported_by_the_hip_build():
    from pydcop_amd.engine import GDBA_REPLICA_SYMBOLS, load_library
    lib = load_library()
    assert lib.mxs_build_kind() == 1
    for name in GDBA_REPLICA_SYMBOLS:
        getattr(lib, name)
