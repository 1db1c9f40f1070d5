"""DPOP on the GPU (pydcop_amd/csrc/dpop.h through the mxs_dpop_* C-ABI) against tests/dpop_oracle.py (pinned
against the reference's own DpopAlgo) and the reference-recorded fixtures: values, costs, UTIL tables and
stats bit for bit, f64 and f32, fused and per-level launches; a 1 024-variable Ising strip (1 023 levels,
65.7 M entries) and a 60-variable colouring (one UTIL of 14.3 M entries)."""
import numpy as np
import pytest

from dpop_common import FUSE, check_golden, compare_dpop, dpop_cases, dpop_golden_files, load_dpop_golden
from pydcop_amd import generators as G
from pydcop_amd.graph import Params

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", dpop_cases(), ids=lambda c: c[0])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_dpop_bit_exact_vs_oracle(case, dtype):
    from dpop_oracle import OracleDpop
    name, make, pkw = case
    compare_dpop(OracleDpop, make(), Params(dtype=dtype, **pkw))


@pytest.mark.parametrize("path", dpop_golden_files(), ids=lambda p: p.rsplit("/", 1)[-1])
def test_dpop_equals_the_reference_fixtures(path):
    from pydcop_amd.dpop import DpopEngine
    g, pkw, tree, ref_idx, ref_cost, utils = load_dpop_golden(path)
    for f in FUSE:
        with DpopEngine(g, Params(**pkw), tree=tree, fuse_entries=f) as e:
            e.solve()
            check_golden(e, ref_idx, ref_cost, utils)


def _measure(g):
    """(depth, widest separator, widest UTIL, all UTIL entries) of build_pseudotree's tree, in plain Python"""
    from pydcop_amd.dpop import build_pseudotree
    parent, crow, cidx = build_pseudotree(g)
    n = g.n_vars
    depth, order = np.zeros(n, dtype=np.int64), []
    stack = [r for r in range(n) if parent[r] < 0]
    while stack:
        v = stack.pop()
        order.append(v)
        for c in cidx[crow[v]:crow[v + 1]]:
            depth[c] = depth[v] + 1
            stack.append(int(c))
    scopes = [[int(u) for u in g.edge_var[g.factor_rowptr[f]:g.factor_rowptr[f + 1]]] for f in range(g.n_factors)]
    sep = [set() for _ in range(n)]
    for s in scopes:
        sep[max(s, key=lambda u: depth[u])].update(s)
    total = widest = widest_sep = 0
    for v in reversed(order):
        sep[v].discard(v)
        if parent[v] >= 0:
            sep[parent[v]].update(sep[v])
            e = int(np.prod([int(g.dom_size[u]) for u in sep[v]], dtype=np.int64))
            total, widest, widest_sep = total + e, max(widest, e), max(widest_sep, len(sep[v]))
    return int(depth.max()), widest_sep, widest, total


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,make,expect", [
    ("ising_8x128", lambda: G.ising_grid(8, 128, seed=1), (1023, 16, 65_536)),
    ("coloring_60", lambda: G.random_coloring(60, avg_degree=3, seed=4), (30, 15, 14_348_907)),
], ids=["ising_8x128", "coloring_60"])
def test_dpop_large_instances(name, make, expect, dtype):
    """idx, cost, the widest UTIL and the UTILs sent to the roots against the numpy oracle, bit for bit;
    stats() equals what the tree measures (a root sends no UTIL, so none is counted for it)"""
    from dpop_oracle import OracleDpop
    g = make()
    depth, widest_sep, widest, total = _measure(g)
    assert (depth, widest_sep, widest) == expect
    ora = compare_dpop(OracleDpop, g, Params(dtype=dtype), fuse=(-1,), all_utils=False)
    st = ora.stats()
    assert (st["depth"], st["widest_separator"], st["widest_util_entries"], st["total_entries"]) == (depth, widest_sep, widest, total)


def test_dpop_large_per_level_launches_equal_fused():
    from pydcop_amd.dpop import DpopEngine
    g = G.ising_grid(8, 128, seed=1)
    out = []
    for f in (0, -1):
        with DpopEngine(g, Params(), fuse_entries=f) as e:
            e.solve()
            out.append((e.state(), e.stats()))
    np.testing.assert_array_equal(out[0][0]["idx"], out[1][0]["idx"])
    np.testing.assert_array_equal(out[0][0]["cost"], out[1][0]["cost"])
    assert out[0][1]["launches_value"] == 1024 and out[1][1]["launches_value"] < 1024


def test_dpop_refuses_over_budget():
    from pydcop_amd.dpop import DpopEngine
    from pydcop_amd.engine import MaxSumGpuError
    with pytest.raises(MaxSumGpuError, match=r"need \d+ bytes.*over the budget"):
        DpopEngine(G.random_coloring(300, avg_degree=2, seed=3), Params())


def test_dpop_library_is_the_hip_build():
    from pydcop_amd.engine import load_library
    lib = load_library()
    assert lib.mxs_build_kind() == 1 and lib.mxs_version() >= 240
    for name in ("mxs_dpop_create", "mxs_dpop_solve", "mxs_dpop_get_state", "mxs_dpop_eval_cost", "mxs_dpop_stats",
                 "mxs_dpop_util_dims", "mxs_dpop_get_util", "mxs_dpop_destroy"):
        getattr(lib, name)
