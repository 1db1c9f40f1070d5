"""The replica engines at several blocks per replica on the emulated engine build (the very same sources, g++ against
the fake HIP runtime, blocks one after another): the CPU twin of tests/test_gpu_replica_shapes.py.  The tests are those
of tests/replica_shapes_common.py, but the one of 4096 replicas: this build takes 8 s (MGM-2) to 80 s (MGM) for it."""
import pytest

from replica_shapes_common import (  # noqa: F401  (collected here)
    test_replicas_equal_their_oracles_at_several_blocks,
    test_best_state_snapshots_span_blocks,
    test_tracked_run_with_three_different_blocks_per_replica,
    test_gdba_best_state_records_beyond_the_first_block_of_the_final_reduction,
    test_ranking_ties_break_on_the_lowest_index)


@pytest.fixture(scope="module")
def lib_path():
    from emu.build_emu import build
    return build()
