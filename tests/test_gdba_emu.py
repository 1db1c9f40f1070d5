"""GDBA on the emulated engine build (the very same mgm.hip / gdba.h, g++ against the fake HIP runtime)
against tests/gdba_oracle.py and the reference-recorded fixtures, bit for bit, round by round -- the
CPU twin of tests/test_gpu_gdba.py."""
import numpy as np
import pytest

from gdba_common import compare_gdba, gdba_cases
from pydcop_amd.graph import Params


@pytest.fixture(scope="module")
def emu_lib():
    from emu.build_emu import build
    return build()


@pytest.mark.parametrize("case", gdba_cases(), ids=lambda c: c[0])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_gdba_emu_bit_exact_vs_oracle(case, dtype, emu_lib):
    from gdba_oracle import OracleGdba
    name, make, pkw, kw = case
    compare_gdba(OracleGdba, make(), Params(dtype=dtype, **pkw), kw, lib_path=emu_lib)


def test_gdba_emu_float_variable_costs_in_index_order(emu_lib):
    """Variable costs that are no dyadic fractions: the cumulative sums run in ascending variable index."""
    from gdba_oracle import OracleGdba
    from pydcop_amd import generators as G
    for dtype in ("f64", "f32"):
        compare_gdba(OracleGdba, G.random_mixed(40, 60, seed=7), Params(dtype=dtype),
                     dict(modifier="M", violation="NM", increase_mode="T", seed=7), lib_path=emu_lib)


def test_gdba_emu_refusals(emu_lib):
    from pydcop_amd import generators as G
    from pydcop_amd.engine import MaxSumGpuError
    from pydcop_amd.gdba import MAX_ROUNDS, GdbaEngine
    g = G.random_coloring(20, avg_degree=1, seed=1)
    for name in ("modifier", "violation", "increase_mode"):
        with pytest.raises(ValueError, match=name):
            GdbaEngine(g, Params(), lib_path=emu_lib, **{name: "X"})
    # the byte budget: the plan is sized before anything is allocated
    with GdbaEngine(g, Params(), increase_mode="C", lib_path=emu_lib) as e:
        need = e.pool_bytes
    assert need > 0
    with pytest.raises(MaxSumGpuError, match="budget"):
        GdbaEngine(g, Params(), increase_mode="C", pool_budget=need - 1, lib_path=emu_lib)
    GdbaEngine(g, Params(), increase_mode="C", pool_budget=need, lib_path=emu_lib).close()
    # a round count past the counters' range
    with GdbaEngine(g, Params(), lib_path=emu_lib) as e:
        e.run(3)
        with pytest.raises(MaxSumGpuError, match="65535"):
            e.run(MAX_ROUNDS - 2)
        assert e.cycle_count == 3
        e.run(2)
    for bad in (np.nan, np.inf, -np.inf):
        h = G.random_coloring(20, seed=1)
        h.tables = h.tables.copy()
        h.tables[3] = bad
        with pytest.raises(MaxSumGpuError, match="tables must be finite"):
            GdbaEngine(h, Params(), lib_path=emu_lib)
        h = G.random_coloring(20, seed=1)
        h.var_cost = h.var_cost.copy()
        h.var_cost[5] = bad
        with pytest.raises(MaxSumGpuError, match="variable costs must be finite"):
            GdbaEngine(h, Params(), lib_path=emu_lib)


def test_gdba_emu_dead_slots_store_nothing(emu_lib):
    """E, R and C keep tables only where the scope is {v} + neighbours(v); T keeps one counter per slot."""
    from gdba_common import stars_paths_unaries
    from gdba_oracle import OracleGdba
    from pydcop_amd.gdba import GdbaEngine
    g = stars_paths_unaries(83)
    o = OracleGdba(g, Params(), increase_mode="C")
    with GdbaEngine(g, Params(), increase_mode="C", lib_path=emu_lib) as e:
        sizes = [len(e.modifiers(s)) for s in range(len(g.var_edges))]
        assert e.pool_bytes == 2 * sum(sizes)
    assert sizes == [len(o.modifiers(s)) for s in range(len(g.var_edges))]
    assert 0 in sizes and 9 in sizes
    with GdbaEngine(g, Params(), increase_mode="T", lib_path=emu_lib) as e:
        assert {len(e.modifiers(s)) for s in range(len(g.var_edges))} <= {0, 1}


def test_gdba_emu_seed_changes_the_run(emu_lib):
    from pydcop_amd import generators as G
    from pydcop_amd.gdba import GdbaEngine
    g = G.random_coloring(200, seed=5)
    a, b = GdbaEngine(g, Params(), seed=1, lib_path=emu_lib), GdbaEngine(g, Params(), seed=2, lib_path=emu_lib)
    a.run(3), b.run(3)
    assert (a.assignment()[0] != b.assignment()[0]).any()
    a.close(), b.close()


@pytest.mark.parametrize("path", __import__("gdba_common").gdba_golden_files(), ids=lambda p: p.rsplit("/", 1)[-1])
def test_gdba_oracle_and_emu_equal_the_reference_fixtures(path, emu_lib):
    """tests/golden/gdba/: what the reference's own computations held after T rounds (tools/make_golden_gdba.py)."""
    from gdba_common import check_golden, load_gdba_golden
    from gdba_oracle import OracleGdba
    from pydcop_amd.gdba import GdbaEngine
    g, pkw, kw, rounds, ref = load_gdba_golden(path)
    o = OracleGdba(g, Params(**pkw), **kw)
    o.run(rounds)
    check_golden(o, ref)
    assert o.moves > 0 and (ref["mod"] != (0 if kw["modifier"] == "A" else 1)).any()
    exact32 = np.array_equal(g.tables.astype(np.float32), g.tables)   # small integers and dyadic costs: every sum
    for dtype in ("f64", "f32") if exact32 else ("f64",):              # of the run is exact in f32 too
        with GdbaEngine(g, Params(dtype=dtype, **pkw), lib_path=emu_lib, **kw) as e:
            e.run(rounds)
            check_golden(e, ref)


def test_gdba_fixtures_cover_the_24_variants():
    import json
    seen = set()
    for path in __import__("gdba_common").gdba_golden_files():
        meta = json.loads(bytes(np.load(path)["meta"]).decode())
        seen.add((meta["gdba"]["modifier"], meta["gdba"]["violation"], meta["gdba"]["increase_mode"], meta["mode"]))
    assert len(seen) == 48
