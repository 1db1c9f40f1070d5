"""Max-Sum's best state and cost trace above the engine, on the emulated build: `solve_flat` / the CLI with `best_every`
and `cost_every`, and a library without the new entry points."""
import json

import numpy as np
import pytest

from pydcop_amd import generators as G
from pydcop_amd.engine import ANYTIME_SYMBOLS, MaxSumEngine, MaxSumGpuError, load_library
from pydcop_amd.graph import Params

INF = float("inf")


@pytest.fixture(scope="module")
def emu_lib():
    from emu.build_emu import build
    return build()


def instance():
    return G.random_coloring(60, seed=31, unary_noise=0)     # integer tables; best state at cycle 30, not the last


def test_solve_flat_with_best_every_returns_the_record(emu_lib):
    from pydcop_amd import api
    g = instance()
    res = api.solve_flat(g, "min", 40, best_every=1, infinity=INF, lib_path=emu_lib)
    with MaxSumEngine(g, Params(), lib_path=emu_lib) as eng:
        eng.track_best(1, INF)
        eng.run(40)
        best, final = eng.best(), eng.eval_cost()
    assert res["best_cycle"] == best["cycle"] == 30 and (res["cost"], res["violation"]) == (best["cost"], best["violations"])
    assert res["assignment"] == {f"v{i}": int(x) for i, x in enumerate(best["idx"])} or \
        list(res["assignment"].values()) == [g.domains[i][int(x)] for i, x in enumerate(best["idx"])]
    assert best["cost"] < final[0] and res["cost_curve"] == [] and res["cycle"] == 40
    plain = api.solve_flat(g, "min", 40, infinity=INF, lib_path=emu_lib)          # without it: the final state, as ever
    assert (plain["cost"], plain["violation"]) == final and "best_cycle" not in plain


@pytest.mark.parametrize("cycles", [40, 30])
def test_cost_every_gives_the_curve_of_the_host_loop(emu_lib, cycles):
    """the curve of ONE tracked run call == run(4) + eval_cost() on a twin engine, bit for bit (30 cycles: the last,
    shorter step included), and the result is still the final state"""
    from pydcop_amd import api
    g = instance()
    res = api.solve_flat(g, "min", cycles, cost_every=4, infinity=INF, lib_path=emu_lib)
    curve, done = [], 0
    with MaxSumEngine(g, Params(), lib_path=emu_lib) as twin:
        while done < cycles:
            n = min(4, cycles - done)
            twin.run(n)
            done += n
            curve.append((done,) + twin.eval_cost(infinity=INF))
        final = twin.eval_cost(infinity=INF)
    assert [c[0] for c in res["cost_curve"]] == [c[0] for c in curve] and all(c[0] > 0 for c in curve)
    assert np.array([c[1] for c in res["cost_curve"]]).tobytes() == np.array([c[1] for c in curve]).tobytes()
    assert [c[2] for c in res["cost_curve"]] == [c[2] for c in curve]
    assert (res["cost"], res["violation"]) == final and "best_cycle" not in res
    both = api.solve_flat(g, "min", cycles, cost_every=4, best_every=4, infinity=INF, lib_path=emu_lib)
    assert both["cost_curve"] == res["cost_curve"] and both["best_cycle"] % 4 == 0
    assert both["cost"] == min(c[1] for c in [(0,) + _start_cost(g, emu_lib)] + curve if c[0] % 4 == 0)


def _start_cost(g, lib):
    with MaxSumEngine(g, Params(), lib_path=lib) as eng:
        return eng.eval_cost(infinity=INF)


def test_refusals(emu_lib):
    from pydcop_amd import api
    g = instance()
    with pytest.raises(ValueError, match="cost_every and best_every"):
        api.solve_flat(g, "min", 8, cost_every=4, best_every=1, lib_path=emu_lib)
    with pytest.raises(ValueError, match="best_every"):
        api.solve_flat(g, "min", 8, algo="amaxsum", best_every=1, lib_path=emu_lib)
    with pytest.raises(ValueError, match="best_every"):
        api.solve_flat(g, "min", 8, algo="mgm", best_every=1, lib_path=emu_lib)
    with pytest.raises(ValueError, match="best_every"):
        api.solve_flat(g, "min", 8, best_every=-1, lib_path=emu_lib)
    with pytest.raises(ValueError, match="best_every"):
        api.solve_flat(g, "min", 8, best_every=1, devices=2, lib_path=emu_lib)


def test_cli_takes_best_every(emu_lib, tmp_path, capsys):
    """`python -m pydcop_amd.api -c 40 -p best_every:1 instance.npz`: solve_flat's result"""
    from pydcop_amd import api, engine
    g = instance()
    path = str(tmp_path / "coloring.npz")
    g.save(path, objective="min")
    before = engine.DEFAULT_LIB
    engine.register_test_engine(emu_lib, make_default=True)
    try:
        api.main(["-c", "40", "-p", "best_every:1", path])
        out = json.loads(capsys.readouterr().out)
        res = api.solve_flat(g, "min", 40, best_every=1, infinity=INF)
    finally:
        engine.DEFAULT_LIB = before
    assert out["status"] == "FINISHED" and out["assignment"] == res["assignment"]
    assert (out["best_cycle"], out["cost"], out["violation"]) == (30, res["cost"], res["violation"])


def test_a_library_without_the_entry_points_says_so(emu_lib, monkeypatch):
    """a library built from older sources loads and runs, and is refused by name for tracking"""
    import pydcop_amd.engine as M

    class Old:
        def __init__(self, lib):
            self._lib, self._name = lib, "libmaxsum_hip_old.so"

        def __getattr__(self, name):
            if name in ANYTIME_SYMBOLS:
                raise AttributeError(name)
            return getattr(self._lib, name)

    monkeypatch.setattr(M, "load_library", lambda path=None: Old(load_library(emu_lib)))
    with MaxSumEngine(instance()) as eng:
        eng.run(3)
        assert eng.cycle_count == 3 and eng.eval_cost()[1] == 0
        with pytest.raises(MaxSumGpuError, match="mxs_track_best"):
            eng.track_best(1)
        with pytest.raises(MaxSumGpuError, match="mxs_get_best"):
            eng.best()
