"""DBA replicas (DbaEngine(replicas=R): R seeded runs in one engine, pydcop_amd/csrc/dba.h) against
tests/dba_oracle.py: replica r is bit for bit OracleDba(seed=seeds[r]) for as long as it runs, weights and stop round
included; the violations counted on the device against dba_common.count_violations of the oracle's state; the ranking
against one computed from the oracles alone; the fixtures recorded from the reference (tests/golden/dba).  Everything
is an integer and compared exactly.  The test functions live here, below the helpers; tests/test_dba_replicas_emu.py
(emulated build) and tests/test_gpu_dba_replicas.py (the HIP library) import them and provide the `lib_path` fixture,
so the two runs cannot drift apart."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from dba_common import STATE_KEYS, check_golden, count_violations, dba_cases, dba_golden_files, load_dba_golden, scaled
from dba_oracle import OracleDba
from gdba_common import stars_paths_unaries
from pydcop_amd import generators as G
from pydcop_amd.dba import DbaEngine
from pydcop_amd.engine import MaxSumGpuError, load_library
from pydcop_amd.graph import Params

MXS_E_INVALID = -1
STEPS = (0, 1, 1, 3, 7)                         # the states after 0, 1, 2, 5 and 12 rounds
HARD_STEPS = (0, 1, 1, 3, 7, 18, 30)            # ... and after 30 and 60
HARD_SEEDS = list(range(5, 13))
HARD_KW = dict(infinity=1000, max_distance=5)
HARD_STOPS = [0, 42, 0, 0, 25, 33, 0, 0]        # of seeds 5..12 within 60 rounds (measured on the oracle)
HARD_VIOLATIONS = [3, 0, 7, 4, 2, 3, 3, 4]      # after 60 rounds, or at the stop


def hard_instance():
    """150 variables: three 64-lane blocks per replica, the last one partial"""
    return G.random_coloring(150, seed=93, variant="hard", unary_noise=0)


def ranking(violations, stops):
    """(violations, stop round with running = +infinity, index): the lexicographic minimum"""
    return min(range(len(violations)), key=lambda r: (violations[r], stops[r] if stops[r] else float("inf"), r))


def oracle_violations(ora, infinity):
    return count_violations(ora.graph, ora.state()["idx"], infinity)


def same_state(eng, oras, what):
    for r, ora in oras.items():
        se, so = eng.state(r), ora.state()
        for k in STATE_KEYS:
            np.testing.assert_array_equal(se[k], so[k], err_msg=f"{k} of replica {r} {what}")
        np.testing.assert_array_equal(eng.weights(r), ora.weights(), err_msg=f"weights of replica {r} {what}")


def same_run(eng, oras, replicas, infinity, what):
    """the stop rounds, the rounds every replica ran, the violations; with every replica checked: the engine's end
    and the ranking"""
    stops, ran, viol = eng.stop_rounds, eng.rounds_of, eng.violations()
    assert len(stops) == len(ran) == len(viol) == replicas
    for r, ora in oras.items():
        assert (stops[r], ran[r]) == (ora.stop_round, ora.cycle_count), (r, what)
        assert viol[r] == oracle_violations(ora, infinity), (r, what)
    if len(oras) == replicas:
        o_stops = [oras[r].stop_round for r in range(replicas)]
        o_viol = [oracle_violations(oras[r], infinity) for r in range(replicas)]
        ended = all(o_stops)
        assert (eng.finished, eng.stop_round) == (ended, max(o_stops) if ended else 0), what
        assert eng.cycle_count == max(o.cycle_count for o in oras.values()), what
        w = ranking(o_viol, o_stops)
        b = eng.best()
        assert (b["replica"], b["stop_round"], b["violations"]) == (w, o_stops[w], o_viol[w]), what
        np.testing.assert_array_equal(b["idx"], oras[w].state()["idx"], err_msg=f"best() {what}")


def compare_replicas(graph, params, kw, replicas, lib_path=None, seed=5, seeds=None, check=None, steps=STEPS, states=None,
                     each_step=None):
    """stop="each": every replica of `check` (default: all) against OracleDba(seed=seeds[r]): every key of STATE_KEYS
    and every weight after the steps, then after reset() and 5 rounds; at every step the stop rounds, the rounds run,
    the violations and best().  `states`: the replicas of `check` whose states and weights are compared (default: all
    of `check`; the others' stop rounds, rounds run and violations still are).  `each_step(oras, rounds)`: called after
    every step, for conditions on the oracle side.  Returns the engine (after those 5 rounds), the oracles' start
    states, and their stop rounds and violations after the steps."""
    eng = DbaEngine(graph, params, seed=seed, seeds=seeds, replicas=replicas, stop="each", lib_path=lib_path, **kw)
    assert eng.replicas == replicas and len(eng.seeds) == replicas
    if seeds is None:
        assert eng.seeds == [seed + r for r in range(replicas)]
    check = list(range(replicas)) if check is None else list(check)
    oras = {r: OracleDba(graph, params, seed=eng.seeds[r], **kw) for r in check}
    watched = oras if states is None else {r: oras[r] for r in states}
    done, starts = 0, None
    for n in steps:
        eng.run(n)
        done += n
        for ora in oras.values():
            ora.run(n)
        same_state(eng, watched, f"after {done} rounds")
        same_run(eng, oras, replicas, kw["infinity"], f"after {done} rounds")
        if each_step is not None:
            each_step(oras, done)
        if starts is None:
            starts = {r: o.state()["idx"] for r, o in oras.items()}
    stops = {r: o.stop_round for r, o in oras.items()}
    viols = {r: oracle_violations(o, kw["infinity"]) for r, o in oras.items()}
    eng.reset()
    assert eng.cycle_count == 0 and not eng.finished and eng.stop_round == 0 and eng.stop_rounds == [0] * replicas
    for ora in oras.values():
        ora.reset()
    same_state(eng, watched, "after reset()")
    eng.run(5)
    for ora in oras.values():
        ora.run(5)
    same_state(eng, watched, "after reset() and 5 rounds")
    same_run(eng, oras, replicas, kw["infinity"], "after reset() and 5 rounds")
    # replica 0 is what the single-state calls mean
    np.testing.assert_array_equal(eng.assignment()[0], eng.assignment(0)[0])
    np.testing.assert_array_equal(eng.weights(), eng.weights(0))
    assert eng.eval_cost() == eng.eval_cost(eng.assignment(0)[0])
    return eng, starts, stops, viols


class ReplicaView:
    """what check_golden reads of an engine, of one replica"""

    def __init__(self, eng, replica):
        self.eng, self.replica = eng, replica

    def state(self):
        return self.eng.state(self.replica)

    def weights(self):
        return self.eng.weights(self.replica)

    @property
    def cycle_count(self):
        return self.eng.rounds_of[self.replica]

    @property
    def stop_round(self):
        return self.eng.stop_rounds[self.replica]

    @property
    def finished(self):
        return self.stop_round != 0


# ---- the tests; `lib_path`: the fixture of the importing file (the emulated build, or None = the HIP library)

def test_every_replica_equals_the_oracle_across_a_partial_block(lib_path):
    """Seeds 5..12 on the hard 150-variable colouring, max_distance 5, 60 rounds.  Measured on the oracle: the stop
    rounds are [0, 42, 0, 0, 25, 33, 0, 0], the violations left [3, 0, 7, 4, 2, 3, 3, 4]: one seed in eight solves
    the instance, and it is not the first to stop."""
    eng, starts, stops, viols = compare_replicas(hard_instance(), Params(), HARD_KW, 8, lib_path=lib_path,
                                                 steps=HARD_STEPS)
    eng.close()
    # what keeps the comparison from passing with the replica fold left out, with one stop word for all replicas or
    # with a ranking by stop round (conditions on the oracle side)
    assert [stops[r] for r in range(8)] == HARD_STOPS
    assert [viols[r] for r in range(8)] == HARD_VIOLATIONS
    assert all((starts[r] != starts[0]).any() for r in range(1, 8))
    w = ranking(HARD_VIOLATIONS, HARD_STOPS)
    assert w == 1 and HARD_VIOLATIONS.count(HARD_VIOLATIONS[w]) == 1
    first = min((s, r) for r, s in enumerate(HARD_STOPS) if s)[1]
    assert first == 4 and first != w


def test_stop_first_ends_every_replica_with_the_first_stop(lib_path):
    """the same instance and seeds under stop="first": the engine ends at round 25 (replica 4's stop), every replica
    having completed it"""
    g, F = hard_instance(), 25
    oras = [OracleDba(g, Params(), seed=s, **HARD_KW) for s in HARD_SEEDS]
    for o in oras:
        o.run(F)
    o_stops = [o.stop_round for o in oras]
    assert o_stops == [0, 0, 0, 0, F, 0, 0, 0]                      # (the oracle side: nobody stops before 25)
    o_viol = [oracle_violations(o, HARD_KW["infinity"]) for o in oras]
    w = ranking(o_viol, o_stops)
    with DbaEngine(g, Params(), seeds=HARD_SEEDS, replicas=8, stop="first", lib_path=lib_path, **HARD_KW) as eng:
        eng.run(60)
        for again in (False, True):
            assert eng.finished and eng.stop_round == F and eng.cycle_count == F
            assert eng.stop_rounds == o_stops and eng.rounds_of == [F] * 8
            same_state(eng, dict(enumerate(oras)), "at the first stop" + " and a further run" * again)
            assert list(eng.violations()) == o_viol
            b = eng.best()
            assert (b["replica"], b["stop_round"], b["violations"]) == (w, o_stops[w], o_viol[w])
            np.testing.assert_array_equal(b["idx"], oras[w].state()["idx"])
            eng.run(10)                                             # after the end: nothing
        # the rounds of one call and of several: the end is the same
        eng.reset()
        for n in (10, 10, 10):
            eng.run(n)
        assert (eng.finished, eng.cycle_count, eng.stop_rounds) == (True, F, o_stops)
        same_state(eng, dict(enumerate(oras)), "at the first stop, in three calls")


@pytest.mark.parametrize("case", dba_cases(), ids=lambda c: c[0])
def test_all_eval_paths_arity3_initial_values_and_name_ranks(case, lib_path):
    """register bounds 4 / 8 / 32 and the wide walk, arity 3, initial values (not looked at), shuffled names"""
    name, make, kw = case
    kw = dict(kw)
    seed = kw.pop("seed")
    replicas = 2 + len(name) % 2
    eng, *_ = compare_replicas(make(), Params(), kw, replicas, lib_path=lib_path, seed=seed)
    eng.close()


@pytest.mark.parametrize("path", dba_golden_files(), ids=lambda p: os.path.basename(p)[:-4])
def test_reference_fixtures(path, lib_path):
    g, kw, rounds, ref, info = load_dba_golden(path)
    kw = dict(kw)
    seed = int(kw.pop("seed"))
    with DbaEngine(g, Params(), seeds=[seed + 1, seed], replicas=2, lib_path=lib_path, **kw) as eng:
        eng.run(rounds)
        check_golden(ReplicaView(eng, 1), ref, info)


def test_fixture_set_is_complete():
    assert len(dba_golden_files()) == 10


def test_many_small_replicas(lib_path):
    """more blocks than one replica needs, and the highest offsets: 64 replicas of 12 variables"""
    eng, *_ = compare_replicas(G.random_coloring(12, seed=31, variant="hard", unary_noise=0), Params(),
                               dict(infinity=1000, max_distance=50), 64, lib_path=lib_path, check=(0, 1, 31, 32, 63))
    eng.close()


def test_explicit_seeds(lib_path):
    seeds = [9, 9, 2 ** 64 - 1, 2 ** 63]
    g = G.random_coloring(45, seed=31, variant="hard", unary_noise=0)
    eng, *_ = compare_replicas(g, Params(), dict(infinity=1000, max_distance=50), 4, lib_path=lib_path, seeds=seeds)
    assert eng.seeds == seeds
    s0, s1 = eng.state(0), eng.state(1)
    for k in STATE_KEYS:                                            # the same seed: the same run, weights included
        np.testing.assert_array_equal(s0[k], s1[k])
    np.testing.assert_array_equal(eng.weights(0), eng.weights(1))
    assert (eng.weights(0) > 1).any()                               # (and something was increased)
    eng.close()
    with DbaEngine(G.random_coloring(10, seed=1), seed=2 ** 64 - 1, replicas=2, lib_path=lib_path) as e:
        assert e.seeds == [2 ** 64 - 1, 0]                          # the default seeds wrap modulo 2**64


def test_one_replica_equals_the_single_run_engine(lib_path):
    """seeds=[s] goes through mxs_dba_create_replicas, seed=s through mxs_dba_create: the same run, the oracle's"""
    g, s = hard_instance(), 9
    kw = dict(infinity=1000, max_distance=5)
    with DbaEngine(g, Params(), seeds=[s], replicas=1, lib_path=lib_path, **kw) as rep, \
            DbaEngine(g, Params(), seed=s, lib_path=lib_path, **kw) as one:
        n = C.c_int32(0)
        for e in (rep, one):
            e._call("replicas", C.byref(n))
            assert n.value == 1 and e.replicas == 1 and e.seeds == [s]
        ora = OracleDba(g, Params(), seed=s, **kw)
        for _ in range(30):                                         # (seed 9 stops in round 25)
            rep.run(1), one.run(1), ora.run(1)
            for k in STATE_KEYS:
                np.testing.assert_array_equal(rep.state()[k], one.state()[k])
                np.testing.assert_array_equal(rep.state()[k], ora.state()[k])
            np.testing.assert_array_equal(rep.weights(), one.weights())
            np.testing.assert_array_equal(rep.weights(), ora.weights())
            for e in (rep, one):
                assert (e.finished, e.stop_round, e.cycle_count) == (ora.finished, ora.stop_round, ora.cycle_count)
                assert (e.stop_rounds, e.rounds_of) == ([ora.stop_round], [ora.cycle_count])
                assert list(e.violations()) == [oracle_violations(ora, 1000)]
        assert ora.stop_round == 25
        # best() of a single run is that run
        b = one.best()
        assert (b["replica"], b["stop_round"], b["violations"]) == (0, 25, oracle_violations(ora, 1000))
        np.testing.assert_array_equal(b["idx"], ora.state()["idx"])
        for e in (one, rep):
            with pytest.raises(MaxSumGpuError, match="replica"):
                e.state(1)
            with pytest.raises(MaxSumGpuError, match="replica"):
                e.weights(1)


def never_playing(g):
    """the variables all of whose constraints are unary, and those constraints"""
    arity = np.diff(g.factor_rowptr)
    plays = np.zeros(g.n_vars, dtype=bool)
    for f in np.flatnonzero(arity > 1):
        plays[g.edge_var[g.factor_rowptr[f]:g.factor_rowptr[f + 1]]] = True
    return [(int(f), int(g.edge_var[g.factor_rowptr[f]])) for f in np.flatnonzero(arity == 1)
            if not plays[g.edge_var[g.factor_rowptr[f]]]]


def test_violations_include_a_variable_that_never_plays(lib_path):
    """a variable with a unary constraint only keeps its start draw: its constraint is in no bit row and must still
    be counted"""
    g, kw, seeds = scaled(stars_paths_unaries(83)), dict(infinity=1000, max_distance=50), list(range(5, 13))
    lone = never_playing(g)
    assert lone
    oras = [OracleDba(g, Params(), seed=s, **kw) for s in seeds]
    at_start = [sum(bool(g.tables[int(g.table_off[f]) + int(o.state()["idx"][v])] >= 1000) for f, v in lone) for o in oras]
    assert any(at_start) and not all(at_start)                      # (the oracle side: it matters, and per replica)
    with DbaEngine(g, Params(), seeds=seeds, replicas=len(seeds), lib_path=lib_path, **kw) as eng:
        for n in (0, 3, 9):
            eng.run(n)
            for o in oras:
                o.run(n)
            assert list(eng.violations()) == [oracle_violations(o, 1000) for o in oras]
            for r, o in enumerate(oras):                            # (still at its start draw)
                assert all(o.state()["idx"][v] == eng.state(r)["idx"][v] for _, v in lone)
        eng.reset()
        for o in oras:
            o.reset()
        assert list(eng.violations()) == [oracle_violations(o, 1000) for o in oras]


# ---- the boundaries of the launches: several blocks of k_dbar_viol_partial (VIOL_CHUNK constraints each) and of the
# wide walk per replica, a second and a third block of k_dbar_viol_final (64 replicas each), the top of the replica
# range, the ranking's ties, stop="first" with the stopper past the first 64 replicas

VIOL_CHUNK = 1024                               # the constraints one block of k_dbar_viol_partial counts
BEYOND_64 = (0, 63, 64, 65, 129)
SMALL_KW = dict(infinity=1000, max_distance=50)


def small_hard():
    return G.random_coloring(12, seed=31, variant="hard", unary_noise=0)


def chunk_violations(g, idx, infinity):
    """the violated constraints of every VIOL_CHUNK constraints in index order: what part[r][b] must hold"""
    counts = [count_violations_of(g, idx, infinity, f0, min(f0 + VIOL_CHUNK, g.n_factors))
              for f0 in range(0, g.n_factors, VIOL_CHUNK)]
    assert sum(counts) == count_violations(g, idx, infinity)
    return counts


def count_violations_of(g, idx, infinity, f0, f1):
    n = 0
    for f in range(f0, f1):
        lin = 0
        for e in range(g.factor_rowptr[f], g.factor_rowptr[f + 1]):
            lin = lin * int(g.dom_size[g.edge_var[e]]) + int(idx[g.edge_var[e]])
        n += bool(g.tables[int(g.table_off[f]) + lin] >= infinity)
    return n


@pytest.mark.parametrize("n_vars,replicas", [(640, 3), (1200, 2)], ids=["two_blocks", "three_blocks"])
def test_violation_partials_of_several_blocks(n_vars, replicas, lib_path):
    """Hard colourings of 1280 and 2400 constraints: part[r][b] with b = 1 and b = 2, the last chunk partial (256 and 352
    constraints).  Measured on the oracle (seeds 5.., max_distance 5): after 0, 1 and 4 rounds every chunk of every
    replica holds violations (at 640 variables [322, 96], [175, 43], [63, 15] for seed 5), and the replicas' counts
    differ chunk by chunk."""
    g = G.random_coloring(n_vars, seed=32, variant="hard", unary_noise=0)
    assert -(-g.n_factors // VIOL_CHUNK) == {640: 2, 1200: 3}[n_vars] and g.n_factors % VIOL_CHUNK >= 200
    seen = []

    def chunks_hold_violations(oras, done):       # (the oracle side) a dropped, doubled or misplaced partial is seen
        counts = {r: chunk_violations(g, o.state()["idx"], 1000) for r, o in oras.items()}
        assert all(min(c) > 0 for c in counts.values()), (done, counts)
        assert any(counts[r][b] != counts[0][b] for r in counts for b in range(len(counts[0]))), (done, counts)
        seen.append(counts)

    eng, *_ = compare_replicas(g, Params(), HARD_KW, replicas, lib_path=lib_path, steps=(0, 1, 3),
                               each_step=chunks_hold_violations)
    eng.close()
    assert len(seen) == 3


WIDE_DOMS = (33, 5, 40, 3, 65, 8, 34)


def wide_instance():
    """72 variables of domains around the word boundaries (33, 34, 40, 65 among them) on a ring with chords, 0 / 1000
    tables at the density of dba_common.binary_big_domains: the wide walk (a domain above 32) at two blocks of 64
    variables per replica"""
    from gdba_common import from_scopes
    n = 72
    doms = [WIDE_DOMS[i % len(WIDE_DOMS)] for i in range(n)]
    scopes = [[i, (i + 1) % n] if i % 2 else [(i + 1) % n, i] for i in range(n)]
    scopes += [[i, (i + 29) % n] for i in range(0, n, 3)]
    g = from_scopes(doms, scopes, np.random.default_rng(96), 0, 2)
    g.tables = 1000.0 * (np.random.default_rng(97).random(g.tables.shape[0]) < 0.85)
    return g


def test_wide_domains_at_two_blocks_per_replica(lib_path):
    g = wide_instance()
    assert g.n_vars > 64 and g.dom_size.max() > 32
    moved = []
    eng, starts, *_ = compare_replicas(g, Params(), SMALL_KW, 3, lib_path=lib_path, steps=(0, 1, 3, 4),
                                       each_step=lambda oras, done: moved.append({r: o.state()["idx"].copy() for r, o in oras.items()}))
    eng.close()
    # (the oracle side) variables of the second block move, and the replicas differ there
    assert all((moved[-1][r][64:] != moved[0][r][64:]).any() for r in range(3))
    assert all((moved[-1][r][64:] != moved[-1][0][64:]).any() for r in (1, 2))


def lone_unary_violations(g, idx, infinity):
    return sum(bool(g.tables[int(g.table_off[f]) + int(idx[v])] >= infinity) for f, v in never_playing(g))


@pytest.mark.parametrize("name", ["small_hard", "never_playing"])
def test_more_than_64_replicas(name, lib_path):
    """130 replicas: a second and a third block of k_dbar_viol_final.  The states and weights of replicas 0, 63, 64, 65
    and 129, the stop rounds, the violations and best() of all 130 against their oracles.  never_playing: variables with
    a unary constraint only, counted in viol_base[r], which differs among the replicas of index 64 and above."""
    g = small_hard() if name == "small_hard" else scaled(stars_paths_unaries(83))

    def base_differs(oras, done):                 # (the oracle side) viol_base[0] for every replica would be seen
        if name == "never_playing":
            base = [lone_unary_violations(g, oras[r].state()["idx"], 1000) for r in range(130)]
            assert never_playing(g) and len(set(base[64:])) > 1 and any(b != base[0] for b in base[64:]), base

    eng, starts, stops, viols = compare_replicas(g, Params(), SMALL_KW, 130, lib_path=lib_path, steps=(0, 1, 3, 8),
                                                 states=BEYOND_64, each_step=base_differs)
    eng.close()
    assert len(set(viols[r] for r in range(64, 130))) > 1           # (the oracle side: the counts past 64 differ)


def test_the_top_of_the_replica_range(lib_path):
    """4096 replicas of 12 variables: replicas 0, 64 and 4095 against their oracles; every replica's violation count
    against count_violations of its own state, best() against the ranking of those counts and the stop rounds"""
    g, R, check = small_hard(), 4096, (0, 64, 4095)
    with DbaEngine(g, Params(), seed=5, replicas=R, stop="each", lib_path=lib_path, **SMALL_KW) as eng:
        oras = {r: OracleDba(g, Params(), seed=5 + r, **SMALL_KW) for r in check}
        done = 0
        for n in (0, 1, 3):
            eng.run(n)
            done += n
            for o in oras.values():
                o.run(n)
            same_state(eng, oras, f"after {done} rounds")
            same_run(eng, oras, R, 1000, f"after {done} rounds")
            states = [eng.state(r)["idx"] for r in range(R)]
            counts = [count_violations(g, idx, 1000) for idx in states]
            assert list(eng.violations()) == counts
            assert len(set(counts)) > 1 and len({s.tobytes() for s in states}) > 64
            stops = eng.stop_rounds
            w, b = ranking(counts, stops), eng.best()
            assert (b["replica"], b["stop_round"], b["violations"]) == (w, stops[w], counts[w])
            np.testing.assert_array_equal(b["idx"], states[w])


TIE_ROUNDS = 60
TIE_ORDERS = [([5, 11, 10, 10, 12], [3, 3, 3, 3, 4], [0, 0, 33, 33, 0], 2),     # seeds, violations, stops, the winner
              ([5, 11, 12], [3, 3, 4], [0, 0, 0], 0)]


@functools.lru_cache(maxsize=None)
def tie_oracle(seed):
    """(violations, stop round, idx) after TIE_ROUNDS rounds on hard_instance(), the oracle's; computed once per seed"""
    o = OracleDba(hard_instance(), Params(), seed=seed, **HARD_KW)
    o.run(TIE_ROUNDS)
    return oracle_violations(o, HARD_KW["infinity"]), o.stop_round, o.state()["idx"].copy()


@pytest.mark.parametrize("order", TIE_ORDERS, ids=["stopped_beats_running", "lowest_index"])
def test_ranking_ties_break_on_the_stop_round_then_the_index(order, lib_path):
    """Equal violations: a run that stopped beats the running ones at lower indices, of two equal entries the lower
    index wins; equal on both keys: the lowest index.  A best_of that ignored the stop round would answer 0 twice."""
    seeds, viol, stops, w = order
    assert [tie_oracle(s)[0] for s in seeds] == viol and [tie_oracle(s)[1] for s in seeds] == stops
    assert ranking(viol, stops) == w and viol.count(viol[w]) > 1 and min(viol) == viol[0] == viol[w]
    with DbaEngine(hard_instance(), Params(), seeds=seeds, replicas=len(seeds), stop="each", lib_path=lib_path,
                   **HARD_KW) as eng:
        eng.run(TIE_ROUNDS)
        assert list(eng.violations()) == viol and eng.stop_rounds == stops
        b = eng.best()
        assert (b["replica"], b["stop_round"], b["violations"]) == (w, stops[w], viol[w]), b
        np.testing.assert_array_equal(b["idx"], tie_oracle(seeds[w])[2])


def test_stop_first_with_the_stopper_past_the_first_64_replicas(lib_path):
    """hard_instance(), seeds 5..70 with seed 30 moved to index 65: 66 replicas, the one that stops first (round 18; the
    next stops would be rounds 24 and 25) in the second block of 64.  Every block of every replica reads the
    engine-wide word: all of them complete round 18 and none runs round 19."""
    g, F, R = hard_instance(), 18, 66
    seeds = list(range(5, 5 + R))
    at = seeds.index(30)
    seeds[at], seeds[R - 1] = seeds[R - 1], seeds[at]
    oras = [OracleDba(g, Params(), seed=s, **HARD_KW) for s in seeds]
    for o in oras:
        o.run(F)
    o_stops = [o.stop_round for o in oras]
    assert o_stops == [0] * (R - 1) + [F]                           # (the oracle side: nobody stops before, one then)
    o_viol = [oracle_violations(o, HARD_KW["infinity"]) for o in oras]
    w = ranking(o_viol, o_stops)
    with DbaEngine(g, Params(), seeds=seeds, replicas=R, stop="first", lib_path=lib_path, **HARD_KW) as eng:
        eng.run(60)
        for again in (False, True):
            what = "at the first stop" + " and a further run" * again
            assert eng.finished and eng.stop_round == F and eng.cycle_count == F, what
            assert eng.stop_rounds == o_stops and eng.rounds_of == [F] * R, what
            same_state(eng, dict(enumerate(oras)), what)
            assert list(eng.violations()) == o_viol, what
            b = eng.best()
            assert (b["replica"], b["stop_round"], b["violations"]) == (w, o_stops[w], o_viol[w]), what
            np.testing.assert_array_equal(b["idx"], oras[w].state()["idx"])
            eng.run(10)                                             # after the end: nothing


def test_refusals(lib_path):
    g = G.random_coloring(12, seed=1)
    for n in (0, 4097):
        with pytest.raises(MaxSumGpuError, match=f"error {MXS_E_INVALID}: .*replicas"):
            DbaEngine(g, replicas=n, lib_path=lib_path)
    with pytest.raises(ValueError, match="seeds"):
        DbaEngine(g, replicas=3, seeds=[1, 2], lib_path=lib_path)
    with pytest.raises(ValueError, match="stop"):
        DbaEngine(g, replicas=2, stop="last", lib_path=lib_path)
    lib = load_library(lib_path)
    cg, cp = g.to_c(), Params().to_c()
    seeds = np.arange(4097, dtype=np.uint64)

    def create(sds, n, policy, graph=cg):
        h = C.c_void_p()
        rc = lib.mxs_dba_create_replicas(C.byref(graph), C.byref(cp), None, 1000.0, 5, sds, n, policy, 0, 0, C.byref(h))
        assert not (rc and h.value)
        return rc, h, lib.mxs_last_error().decode()

    for n in (0, 4097, -3):
        rc, _, msg = create(seeds.ctypes.data, n, 0)
        assert rc == MXS_E_INVALID and "replicas" in msg, n
    rc, _, msg = create(None, 2, 0)
    assert rc == MXS_E_INVALID and "seeds" in msg
    for policy in (2, -1):
        rc, _, msg = create(seeds.ctypes.data, 2, policy)
        assert rc == MXS_E_INVALID and "stop policy" in msg, policy
    rc, h, _ = create(seeds.ctypes.data, 2, 1)
    assert rc == 0 and h.value
    assert lib.mxs_dba_destroy(h) == 0
    # 2^19 + 1 blocks of 64 variables per replica (no constraints: nothing but the domains is stored), 4096 replicas:
    # one block more than 2^31 - 1, refused before anything is allocated
    from pydcop_amd.graph import FlatGraph
    n = 2 ** 19 * 64 + 1
    big = FlatGraph(dom_size=np.ones(n, dtype=np.int32), var_cost=np.zeros(n), factor_rowptr=np.zeros(1, dtype=np.int32),
                    edge_var=np.zeros(0, dtype=np.int32), table_off=np.zeros(1, dtype=np.int64), tables=np.zeros(0),
                    var_rowptr=np.zeros(n + 1, dtype=np.int32), var_edges=np.zeros(0, dtype=np.int32))
    rc, _, msg = create(seeds.ctypes.data, 4096, 0, big.to_c())
    assert rc == MXS_E_INVALID and "too many replicas" in msg
    with pytest.raises(MaxSumGpuError, match=f"error {MXS_E_INVALID}: too many replicas"):
        DbaEngine(big, replicas=4096, lib_path=lib_path)
    with DbaEngine(g, replicas=2, lib_path=lib_path) as e:
        for r in (-1, 2):
            with pytest.raises(MaxSumGpuError, match="replica"):
                e.state(r)
            with pytest.raises(MaxSumGpuError, match="replica"):
                e.weights(r)
        # the int32 bound of the single run holds for the engine's round count
        with pytest.raises(MaxSumGpuError, match=f"error {MXS_E_INVALID}: .*int32"):
            e.run(2 ** 31 - 1)
    # the sticky error is per replica: an infinity too small for the weights (the single run's case), the message
    # names the lowest replica that met it
    from mgm_common import repeated_pairs_and_unaries
    h, kw, sds = scaled(repeated_pairs_and_unaries(30, 87)), dict(infinity=1, max_distance=50), [7, 8, 9]
    raising = []
    for r, s in enumerate(sds):
        try:
            OracleDba(h, Params(), seed=s, **kw).run(3)
        except IndexError:
            raising.append(r)
    assert raising
    with DbaEngine(h, Params(), seeds=sds, replicas=3, lib_path=lib_path, **kw) as e:
        with pytest.raises(MaxSumGpuError, match=f"error -5: .*infinity.*replica {raising[0]}\\)"):
            e.run(3)
    with DbaEngine(g, lib_path=lib_path) as e:                    # best() of a single-run engine: that run
        e.run(3)
        b = e.best()
        assert (b["replica"], b["stop_round"]) == (0, e.stop_round)
        assert b["violations"] == count_violations(g, e.state()["idx"], e.infinity) == e.violations()[0]
