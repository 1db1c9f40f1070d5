"""The replica engines at several blocks per replica on the GPU (dsa.hip, mgm.hip, mgm2.h, gdba.h with replica_cost.h /
replica_host.h): cost partials of a second and a third block, a second and a third block of the final reduction, init
and snapshot kernels over more than 256 variables, launches of one cycle with different blocks per replica, 4096
replicas.  The tests are those of tests/replica_shapes_common.py; tests/test_replica_shapes_emu.py is the CPU twin."""
import pytest

from replica_shapes_common import (  # noqa: F401  (collected here)
    test_replicas_equal_their_oracles_at_several_blocks,
    test_the_top_of_the_replica_range,
    test_best_state_snapshots_span_blocks,
    test_tracked_run_with_three_different_blocks_per_replica,
    test_gdba_best_state_records_beyond_the_first_block_of_the_final_reduction,
    test_ranking_ties_break_on_the_lowest_index)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib_path():
    return None
