"""GDBA's replicas and best state above the engine, on the emulated build: `solve_flat` / the CLI with `restarts` and
`best_every`, and a library without the new entry points."""
import json

import numpy as np
import pytest

from dsa_replicas_common import winner
from gdba_replicas_common import BEST_KW, BEST_ROUNDS, BEST_SEEDS, best_instance, best_records
from pydcop_amd import generators as G
from pydcop_amd.engine import MaxSumGpuError, load_library
from pydcop_amd.gdba import GdbaEngine

INF = 10000.0


@pytest.fixture(scope="module")
def emu_lib():
    from emu.build_emu import build
    return build()


@pytest.fixture(scope="module")
def oracle_side():
    """the records (every = 1) and final states of seeds 5..10, from the oracle alone"""
    records, finals = best_records(1, INF)
    w = winner(records, False)
    assert sum(rec[:2] == records[w][:2] for rec in records) == 1 and records[w][2] < BEST_ROUNDS
    assert (records[w][3] != finals[w][2]).any()                   # not the final state of the winner
    return records, finals, w


def values(g, idx):
    return [g.domains[i][x] for i, x in enumerate(idx)]


def test_solve_flat_returns_the_oracle_derived_winner(emu_lib, oracle_side):
    from pydcop_amd import api
    records, finals, w = oracle_side
    g = best_instance()
    res = api.solve_flat(g, "min", BEST_ROUNDS, algo="gdba", seed=BEST_SEEDS[0], restarts=len(BEST_SEEDS), best_every=1,
                         infinity=INF, lib_path=emu_lib, **BEST_KW)
    assert (res["replica"], res["best_cycle"]) == (w, records[w][2])
    assert [res["assignment"][n] for n in g.var_names] == values(g, records[w][3])
    assert (res["violation"], res["cost"]) == records[w][:2]
    assert res["replica_costs"] == [f[1] for f in finals]           # (the final states' device costs)
    # best_every alone: replica 0's record
    res = api.solve_flat(g, "min", BEST_ROUNDS, algo="gdba", seed=BEST_SEEDS[0], best_every=1, infinity=INF,
                         lib_path=emu_lib, **BEST_KW)
    assert (res["replica"], res["best_cycle"], res["replica_costs"]) == (0, records[0][2], [finals[0][1]])
    assert (res["violation"], res["cost"]) == records[0][:2] and records[0][2] < BEST_ROUNDS
    assert [res["assignment"][n] for n in g.var_names] == values(g, records[0][3])


def test_one_run_without_records_is_todays_result(emu_lib, oracle_side):
    from pydcop_amd import api
    _, finals, _ = oracle_side
    g = best_instance()
    res = api.solve_flat(g, "min", BEST_ROUNDS, algo="gdba", seed=7, restarts=1, best_every=0, infinity=INF,
                         lib_path=emu_lib, **BEST_KW)
    assert not {"replica", "best_cycle", "replica_costs"} & set(res)
    assert (res["violation"], res["cost"]) == finals[2][:2]
    assert [res["assignment"][n] for n in g.var_names] == values(g, finals[2][2])
    assert res == api.solve_flat(g, "min", BEST_ROUNDS, algo="gdba", seed=7, infinity=INF, lib_path=emu_lib, **BEST_KW)


def test_what_stays_refused(emu_lib):
    from pydcop_amd import api
    g = best_instance()
    with pytest.raises(ValueError, match="dsa"):
        api.solve_flat(g, "min", 5, algo="gdba", restarts=2, lib_path=emu_lib)
    with pytest.raises(ValueError, match="gdba.* with best_every >= 1"):
        api.solve_flat(g, "min", 5, algo="gdba", restarts=2, best_every=0, lib_path=emu_lib)
    with pytest.raises(ValueError, match="best_every"):
        api.solve_flat(g, "min", 5, algo="mgm2", restarts=2, best_every=1, lib_path=emu_lib)
    with pytest.raises(ValueError, match="best_every"):
        api.solve_flat(g, "min", 5, algo="gdba", best_every=-1, lib_path=emu_lib)


def test_cli_round_trip_on_an_instance_file(emu_lib, tmp_path, capsys, oracle_side):
    """`python -m pydcop_amd.api -a gdba -p seed:5 -p restarts:6 -p best_every:1 instance.npz`: solve_flat's result"""
    from pydcop_amd import api, engine
    records, finals, w = oracle_side
    g = best_instance()
    path = str(tmp_path / "mixed.npz")
    g.save(path, objective="min")
    before = engine.DEFAULT_LIB
    engine.register_test_engine(emu_lib, make_default=True)
    try:
        api.main(["-a", "gdba", "-c", str(BEST_ROUNDS), "--infinity", "10000", "-p", "modifier:M", "-p", "violation:NM",
                  "-p", "increase_mode:T", "-p", "seed:5", "-p", "restarts:6", "-p", "best_every:1", path])
        out = json.loads(capsys.readouterr().out)
        res = api.solve_flat(g, "min", BEST_ROUNDS, algo="gdba", seed=5, restarts=6, best_every=1, infinity=INF, **BEST_KW)
    finally:
        engine.DEFAULT_LIB = before
    assert out["status"] == "FINISHED" and out["assignment"] == res["assignment"]
    assert (out["replica"], out["best_cycle"], out["replica_costs"], out["cost"], out["violation"]) == (
        res["replica"], res["best_cycle"], res["replica_costs"], res["cost"], res["violation"])
    assert (out["replica"], out["best_cycle"]) == (w, records[w][2])
    assert (out["violation"], out["cost"]) == records[w][:2] and out["replica_costs"] == [f[1] for f in finals]


def test_a_library_without_the_replica_entry_points_says_so(emu_lib, monkeypatch):
    """a library built from older sources loads (the single run works) and is refused by name for replicas"""
    import pydcop_amd.gdba as M

    class Old:
        def __init__(self, lib):
            self._lib, self._name = lib, "libmaxsum_hip_old.so"

        def __getattr__(self, name):
            if name in M.REPLICA_SYMBOLS:
                raise AttributeError(name)
            return getattr(self._lib, name)

    monkeypatch.setattr(M, "load_library", lambda path=None: Old(load_library(emu_lib)))
    g = G.random_coloring(12, seed=1)
    with GdbaEngine(g) as e:
        e.run(2)
        assert np.array_equal(e.state()["idx"], e.assignment()[0]) and len(e.modifiers(0)) <= 1
        with pytest.raises(MaxSumGpuError, match="mxs_gdba_replica_costs"):
            e.replica_costs()
        with pytest.raises(MaxSumGpuError, match="mxs_gdba_track_best"):
            e.track_best(1)
    with pytest.raises(MaxSumGpuError, match="mxs_gdba_create_replicas"):
        GdbaEngine(g, replicas=2)
