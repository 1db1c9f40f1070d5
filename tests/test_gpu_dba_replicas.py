"""DBA replicas on the GPU (pydcop_amd/csrc/dba.h through mxs_dba_create_replicas): every replica against the oracle
bit for bit, weights and stop rounds included, both stop policies, the violations counted on the device against the
oracle's, the ranking, the fixtures recorded from the reference.  The tests are those of
tests/dba_replicas_common.py; tests/test_dba_replicas_emu.py is the CPU twin."""
import pytest

from dba_replicas_common import (  # noqa: F401  (collected here)
    test_every_replica_equals_the_oracle_across_a_partial_block,
    test_stop_first_ends_every_replica_with_the_first_stop,
    test_all_eval_paths_arity3_initial_values_and_name_ranks,
    test_reference_fixtures,
    test_fixture_set_is_complete,
    test_many_small_replicas,
    test_explicit_seeds,
    test_one_replica_equals_the_single_run_engine,
    test_violations_include_a_variable_that_never_plays,
    test_violation_partials_of_several_blocks,
    test_wide_domains_at_two_blocks_per_replica,
    test_more_than_64_replicas,
    test_the_top_of_the_replica_range,
    test_ranking_ties_break_on_the_stop_round_then_the_index,
    test_stop_first_with_the_stopper_past_the_first_64_replicas,
    test_refusals)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib_path():
    return None


def test_dba_replica_symbols_are_exported_by_the_hip_build():
    from pydcop_amd.engine import DBA_REPLICA_SYMBOLS, load_library
    lib = load_library()
    assert lib.mxs_build_kind() == 1
    for name in DBA_REPLICA_SYMBOLS:
        getattr(lib, name)
