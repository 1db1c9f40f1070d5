"""DBA's replicas above the engine, on the emulated build: `solve_flat` / the CLI with `restarts` and `dba_stop`, and a
library without the new entry points."""
import json

import numpy as np
import pytest

from dba_oracle import OracleDba
from dba_replicas_common import (HARD_KW, HARD_SEEDS, HARD_STOPS, HARD_VIOLATIONS, hard_instance, oracle_violations,
                                 ranking)
from pydcop_amd import generators as G
from pydcop_amd.dba import DbaEngine
from pydcop_amd.engine import MaxSumGpuError, load_library
from pydcop_amd.graph import Params

ROUNDS = 60
KW = dict(dba_infinity=HARD_KW["infinity"], max_distance=HARD_KW["max_distance"])


@pytest.fixture(scope="module")
def emu_lib():
    from emu.build_emu import build
    return build()


@pytest.fixture(scope="module")
def oracle_side():
    """per stop policy: (winner, its values, the violations, the stop rounds, the engine's rounds), from the oracles
    of seeds 5..12 alone"""
    g, out = hard_instance(), {}
    for policy, rounds in (("each", ROUNDS), ("first", min(s for s in HARD_STOPS if s))):
        oras = [OracleDba(g, Params(), seed=s, **HARD_KW) for s in HARD_SEEDS]
        for o in oras:
            o.run(rounds)
        stops = [o.stop_round for o in oras]
        viol = [oracle_violations(o, HARD_KW["infinity"]) for o in oras]
        w = ranking(viol, stops)
        out[policy] = (w, oras[w].state()["idx"], viol, stops, rounds)
    assert (out["each"][0], out["each"][2], out["each"][3]) == (1, HARD_VIOLATIONS, HARD_STOPS)
    assert out["first"][3] == [0, 0, 0, 0, 25, 0, 0, 0]
    return out


def values(g, idx):
    if g.var_names is not None and g.domains is not None:
        return {n: g.domains[i][x] for i, (n, x) in enumerate(zip(g.var_names, idx))}
    return {f"v{i}": int(x) for i, x in enumerate(idx)}


@pytest.mark.parametrize("policy", ["first", "each"])
def test_solve_flat_returns_the_oracle_derived_winner(policy, emu_lib, oracle_side):
    from pydcop_amd import api
    w, idx, viol, stops, rounds = oracle_side[policy]
    g = hard_instance()
    kw = {} if policy == "first" else {"dba_stop": "each"}              # ("first" is the default)
    res = api.solve_flat(g, "min", ROUNDS, algo="dba", seed=HARD_SEEDS[0], restarts=len(HARD_SEEDS), infinity=1000.0,
                         lib_path=emu_lib, **KW, **kw)
    assert (res["replica"], res["replica_violations"], res["stop_rounds"]) == (w, viol, stops)
    assert res["assignment"] == values(g, idx)
    assert (res["cycle"], res["finished"]) == (rounds, policy == "first")
    assert res["violation"] == viol[w]                                  # (0 / 1000 tables: eval_cost's == is DBA's >=)


def test_one_run_is_todays_result(emu_lib):
    from pydcop_amd import api
    g = hard_instance()
    ora = OracleDba(g, Params(), seed=9, **HARD_KW)
    ora.run(ROUNDS)
    res = api.solve_flat(g, "min", ROUNDS, algo="dba", seed=9, restarts=1, infinity=1000.0, lib_path=emu_lib, **KW)
    assert set(res) == {"assignment", "cost", "violation", "cycle", "cost_curve", "finished"}
    assert res["assignment"] == values(g, ora.state()["idx"])
    assert (res["cycle"], res["finished"]) == (ora.cycle_count, ora.finished) == (25, True)
    assert res == api.solve_flat(g, "min", ROUNDS, algo="dba", seed=9, infinity=1000.0, lib_path=emu_lib, **KW)
    assert res == api.solve_flat(g, "min", ROUNDS, algo="dba", seed=9, dba_stop="each", infinity=1000.0, lib_path=emu_lib,
                                 **KW)


def test_what_stays_refused(emu_lib):
    from pydcop_amd import api
    g = hard_instance()
    with pytest.raises(ValueError, match="best_every"):
        api.solve_flat(g, "min", 5, algo="dba", restarts=2, best_every=1, lib_path=emu_lib)
    with pytest.raises(ValueError, match="best_every"):
        api.solve_flat(g, "min", 5, algo="dba", best_every=1, lib_path=emu_lib)
    with pytest.raises(ValueError, match="dsa"):
        api.solve_flat(g, "min", 5, algo="mgm", restarts=2, lib_path=emu_lib)
    with pytest.raises(ValueError, match="gdba.* with best_every >= 1"):
        api.solve_flat(g, "min", 5, algo="gdba", restarts=2, lib_path=emu_lib)
    with pytest.raises(ValueError, match="dba_stop"):
        api.solve_flat(g, "min", 5, algo="dba", restarts=2, dba_stop="last", lib_path=emu_lib)


def test_cli_round_trip_on_an_instance_file(emu_lib, tmp_path, capsys, oracle_side):
    """`python -m pydcop_amd.api -a dba -p seed:5 -p restarts:8 -p dba_stop:each instance.npz`: solve_flat's result"""
    from pydcop_amd import api, engine
    w, idx, viol, stops, _ = oracle_side["each"]
    g = hard_instance()
    path = str(tmp_path / "hard.npz")
    g.save(path, objective="min")
    before = engine.DEFAULT_LIB
    engine.register_test_engine(emu_lib, make_default=True)
    try:
        api.main(["-a", "dba", "-c", str(ROUNDS), "--infinity", "1000", "-p", "infinity:1000", "-p", "max_distance:5",
                  "-p", "seed:5", "-p", "restarts:8", "-p", "dba_stop:each", path])
        out = json.loads(capsys.readouterr().out)
        res = api.solve_flat(g, "min", ROUNDS, algo="dba", seed=5, restarts=8, dba_stop="each", infinity=1000.0, **KW)
    finally:
        engine.DEFAULT_LIB = before
    assert out["status"] == "FINISHED" and out["assignment"] == res["assignment"]
    for key in ("replica", "replica_violations", "stop_rounds", "cost", "violation", "cycle"):
        assert out[key] == res[key], key
    assert (out["replica"], out["replica_violations"], out["stop_rounds"], out["cycle"]) == (w, viol, stops, ROUNDS)
    assert out["assignment"] == values(g, idx)


def test_a_library_without_the_replica_entry_points_says_so(emu_lib, monkeypatch):
    """a library built from older sources loads (the single run works) and is refused by name for replicas"""
    import pydcop_amd.dba as M

    class Old:
        def __init__(self, lib):
            self._lib, self._name = lib, "libmaxsum_hip_old.so"

        def __getattr__(self, name):
            if name in M.REPLICA_SYMBOLS:
                raise AttributeError(name)
            return getattr(self._lib, name)

    monkeypatch.setattr(M, "load_library", lambda path=None: Old(load_library(emu_lib)))
    g = G.random_coloring(12, seed=1)
    with DbaEngine(g, infinity=1000) as e:
        e.run(2)
        assert np.array_equal(e.state()["idx"], e.assignment()[0]) and len(e.weights()) == len(g.var_edges)
        with pytest.raises(MaxSumGpuError, match="mxs_dba_replica_violations"):
            e.violations()
        with pytest.raises(MaxSumGpuError, match="mxs_dba_best_replica"):
            e.best()
        with pytest.raises(MaxSumGpuError, match="mxs_dba_stop_rounds"):
            e.stop_rounds
    with pytest.raises(MaxSumGpuError, match="mxs_dba_create_replicas"):
        DbaEngine(g, replicas=2)
    with pytest.raises(MaxSumGpuError, match="mxs_dba_create_replicas"):
        DbaEngine(g, stop="first")
