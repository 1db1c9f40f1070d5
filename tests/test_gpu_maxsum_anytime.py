"""Max-Sum's best state and cost trace on the GPU (pydcop_amd/csrc/anytime.h through mxs_track_best / mxs_get_best /
mxs_get_cost_trace): the records against the oracle-derived ones, under graph replay and eagerly.  The tests are those
of tests/maxsum_anytime_common.py; tests/test_maxsum_anytime_emu.py is the CPU twin.  The large shape is here alone."""
import numpy as np
import pytest

from maxsum_anytime_common import (  # noqa: F401  (collected here)
    test_record_and_trace_equal_the_oracle_derived_ones,
    test_the_result_depends_on_the_sequence_of_cycles_alone,
    test_graph_chunk_does_not_change_the_result,
    test_track_best_again_and_a_short_trace,
    test_a_new_table_restarts_the_record_and_keeps_the_trace,
    test_refusals_change_nothing,
    test_shapes)
from maxsum_anytime_common import INF, tracked
from pydcop_amd import generators as G
from pydcop_amd.engine import MaxSumEngine
from pydcop_amd.graph import Params
from replica_cost_reference import cost_bound

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib_path():
    return None


def test_large_instance_takes_the_grid_stride_path_of_the_cost_kernel(lib_path):
    """300 000 items, more than the 1024 blocks of 256 threads k_eval is launched with: 6 cycles, every = 2"""
    graph, params = G.random_coloring(100_000), Params()
    assert graph.n_vars + graph.n_factors > 1024 * 256
    with tracked(graph, params, 2, INF, lib_path, trace=8) as eng, MaxSumEngine(graph, params) as twin:
        eng.run(6)
        b = eng.best()
        cyc, cost, viol, evals = eng.cost_trace()
        assert cyc.tolist() == [0, 2, 4, 6] and evals == 4
        first = graph.edge_var[graph.factor_rowptr[:-1]].astype(np.int64)      # binary factors, unary variable costs
        second = graph.edge_var[graph.factor_rowptr[:-1] + 1].astype(np.int64)
        voff = np.concatenate(([0], np.cumsum(graph.dom_size.astype(np.int64))))[:-1]
        own = graph.eval_var_cost if graph.eval_var_cost is not None else graph.var_cost
        seen = []
        for k, c in enumerate(cyc.tolist()):
            twin.run(c - twin.cycle_count)
            tc, tv = twin.eval_cost()
            assert np.float64(tc).tobytes() == cost[k:k + 1].tobytes() and tv == viol[k] == 0
            idx = twin.assignment()[0].astype(np.int64)       # the numpy restatement of the sum for this graph
            items = np.concatenate((graph.tables[graph.table_off[:-1] + idx[first] * graph.dom_size[second] + idx[second]],
                                    own[voff + idx]))
            assert abs(cost[k] - float(np.sum(items))) <= 2 * cost_bound(items.size, float(np.abs(items).sum()))
            seen.append((viol[k], cost[k], c, idx))
        best = min(seen, key=lambda t: t[:3])
        assert (b["cycle"], b["cost"], b["violations"]) == (best[2], best[1], best[0])
        np.testing.assert_array_equal(b["idx"], best[3])
        assert np.float64(b["cost"]).tobytes() == np.float64(eng.eval_cost(b["idx"])[0]).tobytes()
