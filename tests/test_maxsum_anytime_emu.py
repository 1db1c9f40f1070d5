"""Max-Sum's best state and cost trace on the emulated engine build (the very same engine.hip and anytime.h, g++
against the fake HIP runtime, which captures no graphs: the eager path): the CPU twin of
tests/test_gpu_maxsum_anytime.py.  The tests are those of tests/maxsum_anytime_common.py."""
import pytest

from maxsum_anytime_common import (  # noqa: F401  (collected here)
    test_record_and_trace_equal_the_oracle_derived_ones,
    test_the_result_depends_on_the_sequence_of_cycles_alone,
    test_graph_chunk_does_not_change_the_result,
    test_track_best_again_and_a_short_trace,
    test_a_new_table_restarts_the_record_and_keeps_the_trace,
    test_refusals_change_nothing,
    test_shapes)


@pytest.fixture(scope="module")
def lib_path():
    from emu.build_emu import build
    return build()
