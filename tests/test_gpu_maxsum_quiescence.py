"""Max-Sum's end condition on the GPU (pydcop_amd/csrc/quiescence.h through mxs_watch_quiescence / mxs_quiescence /
mxs_run_until_quiescent): detection against the oracle-derived cycles, under graph replay and eagerly.  The tests are
those of tests/maxsum_quiescence_common.py; tests/test_maxsum_quiescence_emu.py is the CPU twin.  The parity cases are
those with at most 20 000 edges; the large shape is here alone."""
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
from maxsum_quiescence_common import F32_CASES, parity_names, watching
from pydcop_amd import generators as G
from pydcop_amd.engine import MaxSumEngine
from pydcop_amd.graph import Params

pytestmark = pytest.mark.gpu
MAX_EDGES = 20000


def pytest_generate_tests(metafunc):
    if "case" in metafunc.fixturenames:
        metafunc.parametrize("case", parity_names(MAX_EDGES))
    if "f32_case" in metafunc.fixturenames:
        names = parity_names(MAX_EDGES, F32_CASES)
        assert len(names) >= 10
        metafunc.parametrize("f32_case", names)


@pytest.fixture(scope="module")
def lib_path():
    return None


def test_large_instance_takes_the_grid_stride_path_of_the_counting_kernel(lib_path):
    """4.5 million counters: more 16-byte quads than the 1024 blocks of 4 waves hold lanes, so every wave takes several
    tiles.  The count after each of 3 cycles against the counters a plain engine hands back."""
    graph, params = G.random_coloring(750_000), Params()
    assert 2 * graph.n_edges // 16 > 1024 * 256
    with watching(graph, params, 1, lib_path) as eng, MaxSumEngine(graph, params) as twin:
        for c in (1, 2, 3):
            eng.run(1), twin.run(1)
            _, _, cv, cf = twin.messages()
            got = eng.quiescence()
            assert (got["active"], got["checks"], got["last_check_cycle"]) == (int((cv != 4).sum() + (cf != 4).sum()), c, c)
            assert got["active"] > 0 and not got["quiescent"]
