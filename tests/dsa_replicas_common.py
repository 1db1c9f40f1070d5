"""DSA replicas (DsaEngine(replicas=R): R seeded runs in one engine, pydcop_amd/csrc/dsa.hip) against the oracle:
replica r is bit for bit OracleDsa(seed=seeds[r]); the device cost against eval_cost; the best-state records against
records derived from the oracle alone.  The test functions live here, below the helpers; tests/test_dsa_replicas_emu.py
(emulated build) and tests/test_gpu_dsa_replicas.py (the HIP library) import them and provide the `lib_path` fixture, so
the two runs cannot drift apart."""
import numpy as np
import pytest

from pydcop_amd import generators as G
from pydcop_amd.dsa import DsaEngine
from pydcop_amd.graph import Params
from replica_cost_reference import check_replica_costs

INF = float("inf")


def parity_cases():
    """(id, instance, Params kwargs, DSA kwargs, R, environment): the smallest shapes that cross each boundary"""
    packed = ("packed", lambda: G.random_coloring(45, seed=31), {}, dict(variant="B"), 3)
    packed_f32 = ("packed_f32_max", lambda: G.random_coloring(40, seed=33), {"mode": "max", "dtype": "f32"}, dict(variant="C"), 2)
    mixed = ("pack_and_rest", lambda: G.random_mixed(30, 65, seed=34, dom_choices=(2, 3, 4)), {}, dict(p_mode="arity"), 3)
    cases = [
        packed + ({},),                      # 15 waves of lanes: the last block of a replica is partial
        packed_f32 + ({},),
        ("packed_isolated", lambda: G.random_coloring(60, avg_degree=1, seed=36), {"mode": "max"}, {}, 5, {}),
        mixed + ({},),                       # both kernels in one run
        mixed + ({"MAXSUM_LOCAL_SEARCH_ROWS": "0"},),
        ("slots_d6", lambda: G.meeting_like(10, dom=6), {"mode": "max"}, dict(variant="A", probability=0.9), 4, {}),
        ("slots_d12", lambda: G.meeting_like(8, dom=12), {"mode": "max"}, dict(variant="B", probability=0.8), 4, {}),
        ("slots_d24", lambda: G.meeting_like(6, dom=24), {"mode": "max"}, dict(variant="C", probability=0.6), 4, {}),
        ("csr_walk_d35", lambda: G.meeting_like(5, dom=35), {}, dict(variant="A", probability=0.9), 2, {}),
    ]
    for forced in ("1", "2"):                # the generic kernels on packed-eligible instances
        cases += [packed + ({"MAXSUM_LOCAL_SEARCH_GENERIC": forced},), packed_f32 + ({"MAXSUM_LOCAL_SEARCH_GENERIC": forced},)]
    return cases


def case_id(c):
    return c[0] + "".join(f"-{k[-7:]}{v}" for k, v in c[5].items())


def check_costs(eng, replicas, infinity=INF):
    """replica_costs == eval_cost of every replica's assignment (violations exactly, the cost to the bound of
    compare_dsa: the device folds in another order), the same bits from call to call, and both against the plain
    Python sum of tests/replica_cost_reference.py, to the bound that holds for any summation order"""
    cost, viol = eng.replica_costs(infinity)
    again = eng.replica_costs(infinity)
    assert cost.tobytes() == again[0].tobytes() and viol.tobytes() == again[1].tobytes()
    for r in replicas:
        c, v = eng.eval_cost(eng.assignment(r)[0], infinity)
        assert viol[r] == v, (r, viol[r], v)
        assert abs(cost[r] - c) <= 1e-9 * max(1.0, abs(c)), (r, cost[r], c)
    check_replica_costs(eng, replicas, infinity, cost, viol)
    return cost, viol


def compare_replicas(oracle_cls, graph, params, dsa_kw, replicas, lib_path=None, seed=5, seeds=None, check=None,
                     steps=(0, 1, 1, 3, 10)):
    """every replica of `check` (default: all) against OracleDsa(seed=seeds[r]): values and held costs bit for bit
    after the steps, then after reset() and 4 more cycles"""
    eng = DsaEngine(graph, params, seed=seed, seeds=seeds, replicas=replicas, lib_path=lib_path, **dsa_kw)
    assert eng.replicas == replicas and len(eng.seeds) == replicas
    if seeds is None:
        assert eng.seeds == [seed + r for r in range(replicas)]
    check = list(range(replicas)) if check is None else list(check)
    oras = {r: oracle_cls(graph, params, seed=eng.seeds[r], **dsa_kw) for r in check}

    def same(what):
        for r, ora in oras.items():
            (ie, ce), (io, co) = eng.assignment(r), ora.assignment()
            np.testing.assert_array_equal(ie, io, err_msg=f"values of replica {r} {what}")
            np.testing.assert_array_equal(ce, co, err_msg=f"costs of replica {r} {what}")
        check_costs(eng, check)

    done = 0
    for n in steps:
        eng.run(n)
        done += n
        for ora in oras.values():
            ora.run(n)
            assert eng.cycle_count == ora.cycle_count == done
        same(f"after {done} cycles")
    eng.reset()
    eng.run(4)
    for ora in oras.values():
        ora.reset(), ora.run(4)
    same("after reset() and 4 cycles")
    # replica 0 is what the single-engine calls mean
    np.testing.assert_array_equal(eng.assignment()[0], eng.assignment(0)[0])
    assert eng.eval_cost() == eng.eval_cost(eng.assignment(0)[0])
    for ora in oras.values():
        ora.close()
    return eng


# ---- best state: the expected records from the oracle alone

def better(a, b, is_max):
    """(violations, cost) a strictly better than b"""
    return a[0] < b[0] or (a[0] == b[0] and (a[1] > b[1] if is_max else a[1] < b[1]))


def oracle_records(oracle_cls, graph, params, dsa_kw, seeds, cycles, every, infinity):
    """Per seed: the record (violations, cost, cycle, idx) of a run stepped one cycle at a time -- taken at cycle 0
    and after every cycle c with c % every == 0, replaced on strict improvement only -- and the final (violations,
    cost, idx)."""
    is_max = params.mode == "max"
    records, finals = [], []
    for s in seeds:
        ora = oracle_cls(graph, params, seed=s, **dsa_kw)
        rec = None
        for c in range(cycles + 1):
            if c:
                ora.run(1)
            if c % every == 0:
                idx = ora.assignment()[0].copy()
                cost, viol = ora.eval_cost(idx, infinity)
                if rec is None or better((viol, cost), rec[:2], is_max):
                    rec = (viol, cost, c, idx)
        idx = ora.assignment()[0].copy()
        cost, viol = ora.eval_cost(idx, infinity)
        finals.append((viol, cost, idx))
        records.append(rec)
        ora.close()
    return records, finals


def winner(entries, is_max):
    """the lexicographic minimum of (violations, cost -- negated in max mode --, index)"""
    return min(range(len(entries)), key=lambda r: (entries[r][0], -entries[r][1] if is_max else entries[r][1], r))


def best_cases():
    """(id, instance, Params kwargs, DSA kwargs, infinity, every): integer tables, no variable costs, f64 -- every sum
    is exact, the device ranking cannot differ from the host's"""
    soft = lambda: G.random_coloring(60, seed=31, unary_noise=0)                      # noqa: E731
    hard = lambda: G.random_coloring(60, seed=32, variant="hard", unary_noise=0)      # noqa: E731
    return [("soft_A_every1", soft, {}, dict(variant="A", probability=1.0), INF, 1),
            ("hard_C_every1", hard, {}, dict(variant="C", probability=0.9), 1000.0, 1),
            ("hard_C_every4", hard, {}, dict(variant="C", probability=0.9), 1000.0, 4)]


BEST_SEEDS = list(range(5, 13))
BEST_CYCLES = 24


def compare_best(oracle_cls, case, lib_path=None):
    name, make, kw, dsa_kw, infinity, every = case
    graph, params = make(), Params(**kw)
    is_max = params.mode == "max"
    records, finals = oracle_records(oracle_cls, graph, params, dsa_kw, BEST_SEEDS, BEST_CYCLES, every, infinity)
    # the oracle side first: the case shows what it is there for
    early = [r for r in range(len(BEST_SEEDS))
             if records[r][2] < BEST_CYCLES and better(records[r][:2], finals[r][:2], is_max)]
    assert len(early) >= 4, f"{name}: only {len(early)} of 8 records precede the last cycle and beat the final state"
    if every == 4:
        assert any(rec[2] == 0 for rec in records), "no record of cycle 0 survives"
    eng = DsaEngine(graph, params, seeds=BEST_SEEDS, replicas=len(BEST_SEEDS), lib_path=lib_path, **dsa_kw)
    eng.track_best(every, infinity)
    eng.run(10), eng.run(BEST_CYCLES - 10)        # (records live across calls of run)

    def same_records():
        for r, (viol, cost, cycle, idx) in enumerate(records):
            b = eng.best(r)
            assert (b["replica"], b["violations"], b["cost"], b["cycle"]) == (r, viol, cost, cycle), (r, b, records[r][:3])
            np.testing.assert_array_equal(b["idx"], idx, err_msg=f"snapshot of replica {r}")
        b = eng.best()
        assert b["replica"] == winner(records, is_max)
        np.testing.assert_array_equal(b["idx"], records[b["replica"]][3])

    same_records()
    # reset() clears the records: the same run gives the same records again, not better ones
    eng.reset()
    b0 = eng.best(0)
    assert b0["cycle"] == 0 and np.array_equal(b0["idx"], eng.assignment(0)[0])
    eng.run(BEST_CYCLES)
    same_records()
    # track_best again clears them: the record is the state as it is now
    eng.track_best(every, infinity)
    for r in range(len(BEST_SEEDS)):
        b = eng.best(r)
        assert (b["violations"], b["cost"], b["cycle"]) == (finals[r][0], finals[r][1], BEST_CYCLES)
        np.testing.assert_array_equal(b["idx"], finals[r][2])
    # tracking off: best() ranks the final states
    eng.track_best(0, infinity)
    b = eng.best()
    assert b["replica"] == winner(finals, is_max) and b["cycle"] == BEST_CYCLES
    assert (b["violations"], b["cost"]) == finals[b["replica"]][:2]
    np.testing.assert_array_equal(b["idx"], finals[b["replica"]][2])
    eng.close()
    return records, finals


# ---- the tests; `lib_path`: the fixture of the importing file (the emulated build, or None = the HIP library)

@pytest.mark.parametrize("case", parity_cases(), ids=case_id)
def test_every_replica_equals_the_single_seed_oracle(case, oracle_built, monkeypatch, lib_path):
    from oracle.dsa_oracle import OracleDsa
    name, make, kw, dsa_kw, replicas, env = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    compare_replicas(OracleDsa, make(), Params(**kw), dsa_kw, replicas, lib_path=lib_path).close()


def test_many_small_replicas(oracle_built, lib_path):
    """more blocks than one replica needs, and the highest offsets: 64 replicas, four of them compared"""
    from oracle.dsa_oracle import OracleDsa
    compare_replicas(OracleDsa, G.random_coloring(40, seed=31), Params(), dict(variant="B"), 64, lib_path=lib_path,
                     check=(0, 1, 32, 63)).close()


def test_explicit_seeds(oracle_built, lib_path):
    from oracle.dsa_oracle import OracleDsa
    seeds = [9, 9, 2 ** 64 - 1]
    eng = compare_replicas(OracleDsa, G.random_coloring(45, seed=31), Params(), dict(variant="B"), 3, lib_path=lib_path,
                           seeds=seeds)
    assert eng.seeds == seeds
    for a, b in zip(eng.assignment(0), eng.assignment(1)):      # the same seed: the same run
        np.testing.assert_array_equal(a, b)
    eng.close()
    with DsaEngine(G.random_coloring(10, seed=1), seed=2 ** 64 - 1, replicas=2, lib_path=lib_path) as e:
        assert e.seeds == [2 ** 64 - 1, 0]                        # the default seeds wrap modulo 2**64


def test_replicas_are_distinct_runs(lib_path):
    with DsaEngine(G.random_coloring(100, seed=31), Params(), seed=5, replicas=8, lib_path=lib_path) as eng:
        eng.run(4)
        states = [eng.assignment(r)[0] for r in range(8)]
    assert any((states[r] != states[0]).any() for r in range(1, 8))


def test_device_cost_counts_violations_exactly(lib_path):
    g = G.random_coloring(60, seed=32, variant="hard", unary_noise=0)
    with DsaEngine(g, Params(), variant="C", probability=0.9, seed=5, replicas=8, lib_path=lib_path) as eng:
        for n in (0, 2):
            eng.run(n)
            cost, viol = check_costs(eng, range(8), infinity=1000.0)
            assert (viol > 0).all()
            for r in range(8):                                    # integer tables: both numbers exactly
                assert (cost[r], viol[r]) == eng.eval_cost(eng.assignment(r)[0], 1000.0)


@pytest.mark.parametrize("case", best_cases(), ids=lambda c: c[0])
def test_best_state_records_equal_the_oracle_derived_ones(case, oracle_built, lib_path):
    from oracle.dsa_oracle import OracleDsa
    compare_best(OracleDsa, case, lib_path=lib_path)
