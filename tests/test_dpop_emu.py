"""DPOP on the emulated engine build (the very same mgm.hip / dpop.h, g++ against the fake HIP runtime)
against tests/dpop_oracle.py, bit for bit -- the CPU twin of tests/test_gpu_dpop.py."""
import itertools

import numpy as np
import pytest

from dpop_common import FUSE, check_golden, compare_dpop, dpop_cases, dpop_golden_files, load_dpop_golden
from pydcop_amd import generators as G
from pydcop_amd.graph import Params


@pytest.fixture(scope="module")
def emu_lib():
    from emu.build_emu import build
    return build()


@pytest.mark.parametrize("case", dpop_cases(), ids=lambda c: c[0])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_dpop_emu_bit_exact_vs_oracle(case, dtype, emu_lib):
    """idx, cost, every UTIL and stats(), on the fused and on the per-level launch plan"""
    from dpop_oracle import OracleDpop
    name, make, pkw = case
    compare_dpop(OracleDpop, make(), Params(dtype=dtype, **pkw), lib_path=emu_lib)


@pytest.mark.parametrize("path", dpop_golden_files(), ids=lambda p: p.rsplit("/", 1)[-1])
def test_dpop_oracle_and_emu_equal_the_reference_fixtures(path, emu_lib):
    """tests/golden/dpop/: what the reference's own DpopAlgo objects selected, reported and sent"""
    from dpop_oracle import OracleDpop
    from pydcop_amd.dpop import DpopEngine
    g, pkw, tree, ref_idx, ref_cost, utils = load_dpop_golden(path)
    check_golden(OracleDpop(g, Params(**pkw), tree=tree).solve(), ref_idx, ref_cost, utils)
    for f in FUSE:
        with DpopEngine(g, Params(**pkw), tree=tree, fuse_entries=f, lib_path=emu_lib) as e:
            e.solve()
            check_golden(e, ref_idx, ref_cost, utils)


def test_dpop_fixtures_are_there():
    assert len(dpop_golden_files()) >= 10


def _brute_force(g, is_max=False):
    best = None
    scopes = [g.edge_var[g.factor_rowptr[f]:g.factor_rowptr[f + 1]] for f in range(g.n_factors)]
    tabs = [g.tables[g.table_off[f]:g.table_off[f + 1]].reshape([int(g.dom_size[u]) for u in s]) for f, s in enumerate(scopes)]
    for a in itertools.product(*[range(int(d)) for d in g.dom_size]):
        c = sum(t[tuple(a[u] for u in s)] for s, t in zip(scopes, tabs)) + sum(g.var_cost[g.cost_off[v] + a[v]] for v in range(g.n_vars))
        if best is None or (c > best if is_max else c < best):
            best = c
    return best


@pytest.mark.parametrize("make", [lambda: G.random_coloring(11, avg_degree=3, seed=1), lambda: G.ising_grid(3, 4, seed=2),
                                  lambda: G.random_mixed(9, 10, seed=3)], ids=["coloring_11", "ising_3x4", "mixed_9"])
@pytest.mark.parametrize("mode", ["min", "max"])
def test_dpop_emu_is_the_optimum(make, mode, emu_lib):
    """eval_cost(idx) = the root costs summed = the brute-force optimum"""
    from pydcop_amd.dpop import DpopEngine
    g = make()
    with DpopEngine(g, Params(mode=mode), lib_path=emu_lib) as e:
        e.solve()
        idx, cost = e.assignment()
        roots = e.parent < 0
        total = e.eval_cost(idx)[0]
    opt = _brute_force(g, mode == "max")
    assert total == pytest.approx(opt, rel=1e-12, abs=1e-9)
    assert cost[roots].sum() == pytest.approx(total, rel=1e-12, abs=1e-9)


@pytest.mark.parametrize("case", [c for c in dpop_cases() if c[2].get("mode", "min") == "min"], ids=lambda c: c[0])
def test_dpop_emu_not_worse_than_mgm(case, emu_lib):
    """a min-mode solve: eval_cost(idx) equals the root costs summed and is <= the cost 200 rounds of MGM reach"""
    from pydcop_amd.dpop import DpopEngine
    from pydcop_amd.mgm import MgmEngine
    g = case[1]()
    with DpopEngine(g, Params(), lib_path=emu_lib) as e:
        e.solve()
        idx, cost = e.assignment()
        total = e.eval_cost(idx)[0]
        assert cost[e.parent < 0].sum() == pytest.approx(total, rel=1e-12, abs=1e-9)
    with MgmEngine(g, Params(), lib_path=emu_lib) as m:
        m.run(200)
        local = m.eval_cost()[0]
    print(f"{case[0]}: dpop {total!r}, mgm after 200 rounds {local!r}")
    assert total <= local + 1e-9 * max(1.0, abs(local))


def test_dpop_emu_refuses_over_budget_before_allocating(emu_lib):
    from pydcop_amd.dpop import DpopEngine, build_pseudotree
    from pydcop_amd.engine import MaxSumGpuError
    g = G.random_coloring(300, avg_degree=2, seed=3)
    with pytest.raises(MaxSumGpuError, match=r"need (\d+) bytes.*over the budget of \d+ bytes") as ei:
        DpopEngine(g, Params(), lib_path=emu_lib)     # (terabytes: an allocation of that size would have failed first)
    import re
    assert int(re.search(r"need (\d+) bytes", str(ei.value)).group(1)) > 10 ** 12
    small = G.ising_grid(3, 10, seed=1)
    with DpopEngine(small, Params(), lib_path=emu_lib) as e:
        need = e.stats()["bytes"]
    with pytest.raises(MaxSumGpuError, match=f"need {need} bytes"):
        DpopEngine(small, Params(), max_bytes=need - 1, lib_path=emu_lib)
    with DpopEngine(small, Params(), max_bytes=need, lib_path=emu_lib) as e:
        e.solve()
    with DpopEngine(small, Params(dtype="f32"), max_bytes=need // 2, lib_path=emu_lib) as e:
        e.solve()


def test_dpop_emu_refuses_int32_bound_and_non_finite(emu_lib):
    from pydcop_amd.dpop import DpopEngine
    from pydcop_amd.engine import MaxSumGpuError
    g = G.random_coloring(20, avg_degree=2, seed=1)
    g.tables = g.tables.copy()
    for bad in (np.nan, np.inf, -np.inf):
        g.tables[3] = bad
        with pytest.raises(MaxSumGpuError, match="finite"):
            DpopEngine(g, Params(), lib_path=emu_lib)
    g.tables[3] = 0.0
    rest = float(sum(np.abs(g.tables[g.table_off[f]:g.table_off[f + 1]]).max() for f in range(g.n_factors))
                 + sum(np.abs(g.var_cost[g.cost_off[v]:g.cost_off[v + 1]]).max() for v in range(g.n_vars)))
    first = np.abs(g.tables[g.table_off[0]:g.table_off[1]]).max()
    g.tables[0] = -(2147483647.0 - (rest - first) + 1.0)      # the bound reached, on the negative side
    with pytest.raises(MaxSumGpuError, match="int32"):
        DpopEngine(g, Params(), lib_path=emu_lib)
    g.tables[0] = 1.0e9                                        # well inside
    with DpopEngine(g, Params(), lib_path=emu_lib) as e:
        e.solve()
    g.var_cost = g.var_cost.copy()
    g.var_cost[0] = np.nan
    with pytest.raises(MaxSumGpuError, match="finite"):
        DpopEngine(g, Params(), lib_path=emu_lib)


def test_dpop_emu_refuses_what_is_not_a_pseudo_tree(emu_lib):
    from pydcop_amd.dpop import DpopEngine, build_pseudotree, pack_tree
    from pydcop_amd.engine import MaxSumGpuError
    g = G.ising_grid(3, 4, seed=1)
    n = g.n_vars
    parent, crow, cidx = build_pseudotree(g)
    # a cycle: the root hangs below one of its descendants
    p2 = parent.copy()
    root = int(np.flatnonzero(parent < 0)[0])
    leaf = int([v for v in range(n) if crow[v] == crow[v + 1]][0])
    p2[root] = leaf
    ch = [list(cidx[crow[v]:crow[v + 1]]) for v in range(n)]
    ch[leaf] = ch[leaf] + [root]
    with pytest.raises(MaxSumGpuError, match="not a pseudo-tree"):
        DpopEngine(g, Params(), tree=pack_tree(list(p2), ch), lib_path=emu_lib)
    # a star: acyclic, but a grid's constraints between two leaves lie on no root path
    star = pack_tree([-1] + [0] * (n - 1), [list(range(1, n))] + [[] for _ in range(n - 1)])
    with pytest.raises(MaxSumGpuError, match="not a pseudo-tree.*root path"):
        DpopEngine(g, Params(), tree=star, lib_path=emu_lib)
    # children lists that do not match the parent array
    with pytest.raises(MaxSumGpuError, match="not a pseudo-tree"):
        DpopEngine(g, Params(), tree=(parent, np.zeros(n + 1, dtype=np.int32), np.zeros(0, dtype=np.int32)), lib_path=emu_lib)
    # a chain in index order IS a pseudo-tree of anything: accepted, same optimum
    chain = pack_tree([-1] + list(range(n - 1)), [[v + 1] for v in range(n - 1)] + [[]])
    with DpopEngine(g, Params(), tree=chain, lib_path=emu_lib) as a, DpopEngine(g, Params(), lib_path=emu_lib) as b:
        a.solve(), b.solve()
        assert a.eval_cost()[0] == pytest.approx(b.eval_cost()[0], rel=1e-12)


def test_dpop_emu_custom_tree_matches_oracle(emu_lib):
    """a caller's tree (a chain in index order: separators in another order than the DFS gives)"""
    from dpop_oracle import OracleDpop
    from pydcop_amd.dpop import pack_tree
    g = G.random_mixed(12, 14, seed=21)
    n = g.n_vars
    chain = pack_tree([-1] + list(range(n - 1)), [[v + 1] for v in range(n - 1)] + [[]])
    compare_dpop(OracleDpop, g, Params(), lib_path=emu_lib, tree=chain)


def test_dpop_emu_state_before_solve_is_an_error(emu_lib):
    from pydcop_amd.dpop import DpopEngine
    from pydcop_amd.engine import MaxSumGpuError
    with DpopEngine(G.ising_grid(2, 3, seed=1), Params(), lib_path=emu_lib) as e:
        with pytest.raises(MaxSumGpuError, match="solve"):
            e.state()


def test_solve_flat_dpop_and_the_cli_on_an_instance_file(emu_lib, tmp_path, capsys):
    """`api -a dpop instance.npz`: the optimum, cycle 0, whatever -c says"""
    import json
    from pydcop_amd import api, engine
    from pydcop_amd.dpop import DpopEngine
    g = G.random_coloring(12, avg_degree=2, seed=4)
    with DpopEngine(g, Params(), lib_path=emu_lib) as e:
        e.solve()
        idx, want = e.assignment()[0], e.eval_cost()[0]
    res = api.solve_flat_dpop(g, "min", lib_path=emu_lib)
    assert res["cost"] == want and res["cycle"] == 0 and res["violation"] == 0
    assert [res["assignment"][n] for n in g.var_names] == [g.domains[i][int(x)] for i, x in enumerate(idx)]
    path = str(tmp_path / "inst.npz")
    g.save(path, objective="min")
    before = engine.DEFAULT_LIB
    engine.register_test_engine(emu_lib, make_default=True)
    try:
        capsys.readouterr()
        api.main(["-a", "dpop", "-c", "9", path])
    finally:
        engine.DEFAULT_LIB = before
    out = json.loads(capsys.readouterr().out)
    assert out["cost"] == want and out["cycle"] == 0 and out["assignment"] == res["assignment"]
