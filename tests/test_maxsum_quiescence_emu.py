"""Max-Sum's end condition on the emulated engine build (the very same engine.hip and quiescence.h, g++ against the
fake HIP runtime, which captures no graphs: the eager path): the CPU twin of tests/test_gpu_maxsum_quiescence.py.  The
tests are those of tests/maxsum_quiescence_common.py; the parity cases are those with at most 2000 edges."""
import pytest

from maxsum_quiescence_common import (  # noqa: F401  (collected here)
    test_the_oracle_ends_on_most_parity_cases,
    test_detection_equals_the_oracles_f64,
    test_detection_equals_the_oracles_f32,
    test_active_per_check,
    test_wider_periods_replay_and_splitting,
    test_never_quiescent,
    test_invalidation,
    test_together_with_track_best,
    test_refusals_change_nothing,
    test_debug_timeline_is_refused_while_watching,
    test_step_calls_are_refused_while_watching,
    test_halo_setup_is_refused_while_watching,
    test_a_sharded_engine_is_refused,
    test_lifecycle,
    test_dynamic_maxsum_forwards_and_a_scope_change_keeps_watching)
from maxsum_quiescence_common import F32_CASES, parity_names

MAX_EDGES = 2000


def pytest_generate_tests(metafunc):
    if "case" in metafunc.fixturenames:
        metafunc.parametrize("case", parity_names(MAX_EDGES))
    if "f32_case" in metafunc.fixturenames:
        metafunc.parametrize("f32_case", parity_names(MAX_EDGES, F32_CASES))


@pytest.fixture(scope="module")
def lib_path():
    from emu.build_emu import build
    return build()
