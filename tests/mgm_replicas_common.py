"""MGM with keyed draws and replicas (MgmEngine(draws="keyed", replicas=R): R seeded runs in one engine,
pydcop_amd/csrc/mgm.hip) against tests/mgm_keyed_oracle.py: replica r is bit for bit the oracle with seed seeds[r]; the
device cost against eval_cost; the best replica against the winner derived from the oracle alone; the fixtures recorded
from the reference (tests/golden/mgm_keyed).  The test functions live here, below the helpers;
tests/test_mgm_replicas_emu.py (emulated build) and tests/test_gpu_mgm_replicas.py (the HIP library) import them and
provide the `lib_path` fixture, so the two runs cannot drift apart."""
import glob
import json
import os

import numpy as np
import pytest

import mgm_common
from dsa_replicas_common import check_costs, winner
from mgm_keyed_oracle import OracleMgmKeyed
from pydcop_amd import generators as G
from pydcop_amd.graph import FlatGraph, Params
from pydcop_amd.mgm import MgmEngine

KEYS = ("idx", "has_cost", "cost", "gain", "new")
HARD = "packed_hard"


def parity_cases():
    """(id, instance, Params kwargs, R, environment): the smallest shapes that cross each boundary"""
    packed = (HARD, lambda: G.random_coloring(45, seed=31, variant="hard"), {}, 3)   # 1000 * I tables: exact ties
    packed_f32 = ("packed_f32_max", lambda: G.random_coloring(40, seed=33), {"mode": "max", "dtype": "f32"}, 2)
    cases = [
        packed + ({},),                      # the last block of a replica's lanes is partial
        packed_f32 + ({},),
        ("packed_isolated", lambda: G.random_coloring(60, avg_degree=1, seed=36), {"mode": "max"}, 5, {}),
        ("pack_and_rest", lambda: G.random_mixed(30, 65, seed=34, dom_choices=(2, 3, 4)), {}, 3, {}),   # both families
        ("slots_d6", lambda: G.meeting_like(10, dom=6), {"mode": "max"}, 3, {}),
        ("slots_d12", lambda: G.meeting_like(8, dom=12), {"mode": "max"}, 3, {}),
        ("slots_d24", lambda: G.meeting_like(6, dom=24), {}, 3, {}),
        ("csr_walk_d35", lambda: G.meeting_like(5, dom=35), {"mode": "max"}, 2, {}),
        ("with_init", lambda: mgm_common.with_init(G.random_coloring(45, seed=37, variant="hard"), 37), {}, 3, {}),
        ("with_init_rest", lambda: mgm_common.with_init(G.random_mixed(30, 65, seed=38, dom_choices=(2, 3, 4)), 38),
         {"mode": "max"}, 2, {}),
    ]
    for forced in ("1", "2"):                # the generic kernels on packed-eligible instances
        cases += [packed + ({"MAXSUM_LOCAL_SEARCH_GENERIC": forced},), packed_f32 + ({"MAXSUM_LOCAL_SEARCH_GENERIC": forced},)]
    return cases


def case_id(c):
    return c[0] + "".join(f"-{k[-7:]}{v}" for k, v in c[4].items())


def same_state(eng, oras, what):
    for r, ora in oras.items():
        se, so = eng.state(r), ora.state()
        for k in KEYS:
            np.testing.assert_array_equal(se[k], so[k], err_msg=f"{k} of replica {r} {what}")


def compare_replicas(graph, params, replicas, lib_path=None, seed=5, seeds=None, check=None, steps=(0, 1, 1, 3, 10)):
    """every replica of `check` (default: all) against OracleMgmKeyed(seed=seeds[r]): the whole state bit for bit after
    the steps, then after reset() and 4 more rounds.  Returns the engine and the oracles, both after those 4 rounds."""
    eng = MgmEngine(graph, params, draws="keyed", seed=seed, seeds=seeds, replicas=replicas, lib_path=lib_path)
    assert eng.replicas == replicas and len(eng.seeds) == replicas
    if seeds is None:
        assert eng.seeds == [seed + r for r in range(replicas)]
    check = list(range(replicas)) if check is None else list(check)
    oras = {r: OracleMgmKeyed(graph, params, draws="keyed", seed=eng.seeds[r]) for r in check}
    done = 0
    starts, finals = None, None
    for n in steps:
        eng.run(n)
        done += n
        for ora in oras.values():
            ora.run(n)
            assert eng.cycle_count == ora.cycle_count == done
        same_state(eng, oras, f"after {done} rounds")
        check_costs(eng, check)
        if starts is None:
            starts = {r: o.state()["idx"] for r, o in oras.items()}
    finals = {r: o.state()["idx"] for r, o in oras.items()}
    late = sum(o.late_picks for o in oras.values())
    eng.reset()
    eng.run(4)
    for ora in oras.values():
        ora.reset(), ora.run(4)
    same_state(eng, oras, "after reset() and 4 rounds")
    # replica 0 is what the single-state calls mean
    np.testing.assert_array_equal(eng.assignment()[0], eng.assignment(0)[0])
    assert eng.eval_cost() == eng.eval_cost(eng.assignment(0)[0])
    return eng, oras, starts, finals, late


def golden_files():
    return sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mgm_keyed", "*.npz")))


def load_golden(path):
    """tools/make_golden_mgm_keyed.py -> (FlatGraph, Params kwargs, seed, rounds, ref): ref holds what the reference's
    own computations held after `rounds` rounds under the keyed draws -- idx, cost (NaN: still None)"""
    z = np.load(path)
    meta = json.loads(bytes(z["meta"]).decode())
    g = FlatGraph(dom_size=z["dom_size"], var_cost=z["var_cost"], factor_rowptr=z["factor_rowptr"],
                  edge_var=z["edge_var"], table_off=z["table_off"], tables=z["tables"],
                  var_rowptr=z["var_rowptr"], var_edges=z["var_edges"],
                  init_idx=z["init_idx"] if "init_idx" in z.files else None)
    g.var_names = meta["var_names"]
    return g.validate(), meta["kwargs"], meta["seed"], meta["rounds"], {"idx": z["ref_idx"], "cost": z["ref_cost"]}


def check_golden(state, ref):
    np.testing.assert_array_equal(state["idx"], ref["idx"])
    held = ~np.isnan(ref["cost"])
    np.testing.assert_array_equal(state["has_cost"].astype(bool), held)
    np.testing.assert_array_equal(state["cost"][held], ref["cost"][held])


# ---- the tests; `lib_path`: the fixture of the importing file (the emulated build, or None = the HIP library)

@pytest.mark.parametrize("case", parity_cases(), ids=case_id)
def test_every_replica_equals_the_keyed_oracle(case, monkeypatch, lib_path):
    name, make, kw, replicas, env = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng, oras, starts, finals, late = compare_replicas(make(), Params(**kw), replicas, lib_path=lib_path)
    eng.close()
    if name == HARD:
        # what keeps the comparison from passing with the draws left out (conditions on the oracle side): a draw of
        # id 11 picked beyond the first value, the replicas start apart and end apart
        assert late >= 1
        assert any((starts[r] != starts[0]).any() for r in starts)
        assert any((finals[r] != finals[0]).any() for r in finals)


def test_many_small_replicas(lib_path):
    """more blocks than one replica needs, and the highest offsets: 64 replicas of 12 variables"""
    eng, *_ = compare_replicas(G.random_coloring(12, seed=31, variant="hard"), Params(), 64, lib_path=lib_path,
                               check=(0, 1, 31, 32, 63))
    eng.close()


def test_explicit_seeds(lib_path):
    seeds = [9, 9, 2 ** 64 - 1, 2 ** 63]
    eng, *_ = compare_replicas(G.random_coloring(45, seed=31, variant="hard"), Params(), 4, lib_path=lib_path, seeds=seeds)
    assert eng.seeds == seeds
    s0, s1 = eng.state(0), eng.state(1)
    for k in KEYS:                                                 # the same seed: the same run
        np.testing.assert_array_equal(s0[k], s1[k])
    eng.close()
    with MgmEngine(G.random_coloring(10, seed=1), draws="keyed", seed=2 ** 64 - 1, replicas=2, lib_path=lib_path) as e:
        assert e.seeds == [2 ** 64 - 1, 0]                         # the default seeds wrap modulo 2**64


def test_device_costs_and_the_best_replica(lib_path):
    """on the hard colouring (integer tables, no variable costs) with infinity = 1000 both numbers are exact; best() is
    the winner derived from the oracle's final states alone"""
    g = G.random_coloring(45, seed=31, variant="hard", unary_noise=0)
    seeds = list(range(5, 13))
    finals = []
    for s in seeds:
        o = OracleMgmKeyed(g, Params(), draws="keyed", seed=s)
        o.run(12)
        idx = o.state()["idx"]
        cost, viol = o.eval_cost(idx, 1000.0)
        finals.append((viol, cost, idx))
    assert len({f[:2] for f in finals}) > 1                        # the ranking has something to rank
    with MgmEngine(g, Params(), draws="keyed", seeds=seeds, replicas=len(seeds), lib_path=lib_path) as eng:
        for n in (0, 12):
            eng.run(n)
            cost, viol = check_costs(eng, range(len(seeds)), infinity=1000.0)
            for r in range(len(seeds)):
                assert (cost[r], viol[r]) == eng.eval_cost(eng.assignment(r)[0], 1000.0)
        assert (viol > 0).any()
        for r, (v, c, idx) in enumerate(finals):
            assert (viol[r], cost[r]) == (v, c)
        b = eng.best(1000.0)
        w = winner(finals, False)
        assert (b["replica"], b["violations"], b["cost"]) == (w, finals[w][0], finals[w][1])
        np.testing.assert_array_equal(b["idx"], finals[w][2])
    # max mode, float tables and variable costs: the cost to rounding, the ranking on the negated cost
    g = G.random_coloring(40, seed=33)
    with MgmEngine(g, Params(mode="max"), draws="keyed", seed=3, replicas=6, lib_path=lib_path) as eng:
        eng.run(8)
        cost, viol = check_costs(eng, range(6))
        b = eng.best()
        assert b["replica"] == winner([(viol[r], cost[r]) for r in range(6)], True)


def test_keyed_single_run_differs_from_the_fixed_draws(lib_path):
    g = G.random_coloring(45, seed=31, variant="hard")
    with MgmEngine(g, Params(), draws="keyed", replicas=1, seed=5, lib_path=lib_path) as k, \
            MgmEngine(g, Params(), lib_path=lib_path) as f:
        plays = OracleMgmKeyed(g).has_nb                       # (the others start at their own optimum in both)
        assert (k.state()["idx"] != f.state()["idx"]).any() and (f.state()["idx"][plays] == 0).all()
        np.testing.assert_array_equal(k.state()["idx"][~plays], f.state()["idx"][~plays])
        k.run(6), f.run(6)
        assert (k.state()["idx"] != f.state()["idx"]).any()
        with pytest.raises(ValueError, match="keyed"):
            f.replica_costs()


@pytest.mark.parametrize("case", [c for c in mgm_common.mgm_cases() if c[0] in ("coloring_hard_ties", "mixed_arity3_max",
                                                                                "meeting_d12", "meeting_d35")],
                         ids=lambda c: c[0])
def test_fixed_draws_still_equal_the_c_oracle(case, oracle_built, lib_path):
    from oracle.mgm_oracle import OracleMgm
    name, make, kw = case
    mgm_common.compare_mgm(OracleMgm, make(), Params(**kw), lib_path=lib_path, steps=(0, 1, 3, 6))


@pytest.mark.parametrize("path", golden_files(), ids=lambda p: os.path.basename(p)[:-4])
def test_reference_fixtures(path, lib_path):
    g, kw, seed, rounds, ref = load_golden(path)
    o = OracleMgmKeyed(g, Params(**kw), draws="keyed", seed=seed)
    o.run(rounds)
    check_golden(o.state(), ref)
    with MgmEngine(g, Params(**kw), draws="keyed", seeds=[seed + 1, seed], replicas=2, lib_path=lib_path) as eng:
        eng.run(rounds)
        check_golden(eng.state(1), ref)


def test_fixture_set_is_complete():
    assert 4 <= len(golden_files()) <= 6
