"""Max-Sum's end condition above the engine, on the emulated build: `solve_flat` / the CLI with `until_quiescent`, the
cap, the combination with `best_every` / `cost_every`, and the refusals."""
import json

import numpy as np
import pytest

from pydcop_amd import generators as G
from pydcop_amd.engine import MaxSumEngine
from pydcop_amd.graph import Params

INF = float("inf")


@pytest.fixture(scope="module")
def emu_lib():
    from emu.build_emu import build
    return build()


def instance():
    return G.random_coloring(60, seed=31, unary_noise=0)     # the first silent cycle is 72 (the oracle's, tests/maxsum_quiescence_common.py)


@pytest.mark.parametrize("every, at", [(1, 72), (4, 73)])
def test_until_quiescent_ends_the_run(emu_lib, every, at):
    from pydcop_amd import api
    g = instance()
    res = api.solve_flat(g, "min", 500, until_quiescent=every, infinity=INF, lib_path=emu_lib)
    assert (res["quiescent"], res["quiescent_cycle"], res["active_edges"]) == (True, at, 0)
    assert res["cycle"] == 128 and res["cost_curve"] == []          # spans of the default 64 cycles
    with MaxSumEngine(g, Params(), lib_path=emu_lib) as eng:        # ... and the state is that of any number of cycles >= 72
        eng.run(500)
        idx, final = eng.assignment()[0], eng.eval_cost()
    assert (res["cost"], res["violation"]) == final
    assert list(res["assignment"].values()) == [int(x) for x in idx] or \
        list(res["assignment"].values()) == [g.domains[i][int(x)] for i, x in enumerate(idx)]


def test_the_cap_comes_first(emu_lib):
    from pydcop_amd import api
    g = instance()
    res = api.solve_flat(g, "min", 50, until_quiescent=1, infinity=INF, lib_path=emu_lib)
    plain = api.solve_flat(g, "min", 50, infinity=INF, lib_path=emu_lib)
    assert (res["quiescent"], res["quiescent_cycle"], res["cycle"]) == (False, None, 50) and res["active_edges"] > 0
    assert (res["cost"], res["violation"], res["assignment"]) == (plain["cost"], plain["violation"], plain["assignment"])
    assert not {"quiescent", "quiescent_cycle", "active_edges"} & set(plain)


def test_together_with_best_every_the_curve_ends_where_the_run_ends(emu_lib):
    from pydcop_amd import api
    g = instance()
    res = api.solve_flat(g, "min", 500, until_quiescent=1, best_every=5, cost_every=5, infinity=INF, lib_path=emu_lib)
    want = api.solve_flat(g, "min", 128, best_every=5, cost_every=5, infinity=INF, lib_path=emu_lib)
    assert res["quiescent_cycle"] == 72 and res["cycle"] == 128
    assert [c[0] for c in res["cost_curve"]] == list(range(5, 126, 5)) + [128]
    assert res["cost_curve"] == want["cost_curve"] and res["best_cycle"] == want["best_cycle"]
    assert (res["cost"], res["violation"], res["assignment"]) == (want["cost"], want["violation"], want["assignment"])
    capped = api.solve_flat(g, "min", 40, until_quiescent=3, cost_every=4, infinity=INF, lib_path=emu_lib)
    assert capped["cycle"] == 40 and not capped["quiescent"] and [c[0] for c in capped["cost_curve"]] == list(range(4, 41, 4))


def test_refusals():
    from pydcop_amd import api
    g = instance()
    for algo in ("amaxsum", "dsa", "mgm", "mgm2", "gdba", "dba"):
        with pytest.raises(ValueError, match="until_quiescent"):
            api.solve_flat(g, "min", 10, until_quiescent=1, algo=algo)
    with pytest.raises(ValueError, match="until_quiescent"):
        api.solve_flat(g, "min", 10, until_quiescent=1, devices=2)
    with pytest.raises(ValueError, match="until_quiescent"):
        api.solve_flat(g, "min", 10, until_quiescent=-1)


def test_the_command_line(emu_lib, tmp_path, capsys):
    """`python -m pydcop_amd.api -c 500 --until_quiescent 1 instance.npz`: solve_flat's result"""
    from pydcop_amd import api, engine
    g = instance()
    path = str(tmp_path / "coloring.npz")
    g.save(path, objective="min")
    before = engine.DEFAULT_LIB
    engine.register_test_engine(emu_lib, make_default=True)
    try:
        api.main(["-c", "500", "--until_quiescent", "1", path])
        out = json.loads(capsys.readouterr().out)
    finally:
        engine.DEFAULT_LIB = before
    assert (out["quiescent"], out["quiescent_cycle"], out["active_edges"], out["cycle"]) == (True, 72, 0, 128)
