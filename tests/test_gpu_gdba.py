"""GDBA on the GPU (pydcop_amd/csrc/gdba.h through the mxs_gdba_* C-ABI) against tests/gdba_oracle.py
(pinned against the reference's own GdbaComputation) and the reference-recorded fixtures: values, held
costs, improvements, new values and every stored modifier table bit for bit, round by round, the 24
variants in min and max, f64 and f32; the 100k-variable colouring; `api -a gdba`."""
import json

import numpy as np
import pytest

from gdba_common import compare_gdba, gdba_cases, same_modifiers, same_state
from pydcop_amd import generators as G
from pydcop_amd.graph import Params

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", gdba_cases(), ids=lambda c: c[0])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_gdba_bit_exact_vs_oracle(case, dtype):
    from gdba_oracle import OracleGdba
    name, make, pkw, kw = case
    compare_gdba(OracleGdba, make(), Params(dtype=dtype, **pkw), kw)


def test_gdba_float_variable_costs_in_index_order():
    from gdba_oracle import OracleGdba
    for dtype in ("f64", "f32"):
        compare_gdba(OracleGdba, G.random_mixed(40, 60, seed=7), Params(dtype=dtype),
                     dict(modifier="M", violation="NM", increase_mode="T", seed=7))


def test_gdba_100k_coloring():
    """coloring_100k (variable costs included), 30 rounds; the state after 1, 2, 10 and 30, the modifier tables of
    a sample of slots and the sum of all of them through the cost they add."""
    from gdba_oracle import OracleGdba
    from pydcop_amd.gdba import GdbaEngine
    g = G.random_coloring(100_000, seed=0, names=False)
    p = Params()
    kw = dict(modifier="A", violation="NZ", increase_mode="E", seed=9)
    with GdbaEngine(g, p, **kw) as eng:
        ora = OracleGdba(g, p, **kw)
        start = eng.eval_cost()[0]
        for n in (1, 1, 8, 20):
            eng.run(n), ora.run(n)
            same_state(eng, ora, f"after {ora.cycle_count} rounds")
        stored = np.flatnonzero(ora.mod_off[:ora.nS] >= 0)
        touched = [s for s in stored if (ora.modifiers(s) != 0).any()]
        assert len(stored) > 1000 and len(touched) > 10
        for s in list(stored[:50]) + touched[:50]:
            np.testing.assert_array_equal(eng.modifiers(int(s)), ora.modifiers(int(s)), err_msg=f"slot {s}")
        assert eng.eval_cost()[0] < 0.7 * start


@pytest.mark.parametrize("mode", ["R", "C", "T"])
def test_gdba_5k_sparse_heavier_modes(mode):
    """More than one block, rows and slabs written by a wave's lanes (domains of 5: slabs of 5 and 25 entries)"""
    from gdba_oracle import OracleGdba
    from pydcop_amd.gdba import GdbaEngine
    g = G.random_coloring(5000, avg_degree=2, n_colors=5, seed=4, names=False, unary_noise=0)
    kw = dict(modifier="M", violation="NM", increase_mode=mode, seed=4)
    with GdbaEngine(g, Params(dtype="f32"), **kw) as eng:
        ora = OracleGdba(g, Params(dtype="f32"), **kw)
        eng.run(15), ora.run(15)
        same_state(eng, ora, "after 15 rounds")
        same_modifiers(eng, ora, "after 15 rounds")
        assert ora.pool[:ora.pool_size].any()


def test_gdba_library_is_the_hip_build():
    from pydcop_amd.engine import ABI_SYMBOLS, load_library
    lib = load_library()
    assert lib.mxs_build_kind() == 1 and lib.mxs_version() >= 250
    for name in ABI_SYMBOLS:
        if name.startswith("mxs_gdba_"):
            getattr(lib, name)
    assert sum(n.startswith("mxs_gdba_") for n in ABI_SYMBOLS) == 8


@pytest.mark.parametrize("path", __import__("gdba_common").gdba_golden_files(), ids=lambda p: p.rsplit("/", 1)[-1])
def test_gdba_equals_the_reference_fixtures(path):
    """tests/golden/gdba/: what the reference's own computations held after T rounds."""
    from gdba_common import check_golden, load_gdba_golden
    from pydcop_amd.gdba import GdbaEngine
    g, pkw, kw, rounds, ref = load_gdba_golden(path)
    exact32 = np.array_equal(g.tables.astype(np.float32), g.tables)
    for dtype in ("f64", "f32") if exact32 else ("f64",):
        with GdbaEngine(g, Params(dtype=dtype, **pkw), **kw) as e:
            e.run(rounds)
            check_golden(e, ref)


def test_api_runs_gdba_end_to_end(tmp_path, capsys):
    """`python -m pydcop_amd.api -a gdba` on an instance file: no pyDCOP import, the engine's own cost."""
    from gdba_oracle import OracleGdba
    from pydcop_amd import api
    g = G.random_coloring(400, avg_degree=2, seed=6, unary_noise=0)
    path = str(tmp_path / "inst.npz")
    g.save(path, objective="min")
    api.main(["-a", "gdba", "-c", "9", "-p", "modifier:M", "-p", "violation:NM", "-p", "increase_mode:R", "-p", "seed:2",
              path])
    out = json.loads(capsys.readouterr().out)
    o = OracleGdba(g, Params(), modifier="M", violation="NM", increase_mode="R", seed=2)
    o.run(9)
    assert out["status"] == "FINISHED" and out["cycle"] == 9
    assert out["cost"] == pytest.approx(o.eval_cost()[0])
    assert [out["assignment"][n] for n in g.var_names] == [int(x) for x in o.state()["idx"]]
