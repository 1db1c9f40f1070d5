"""Max-Sum's end condition detected on the device (MaxSumEngine.watch_quiescence / quiescence / run_until_quiescent,
pydcop_amd/csrc/quiescence.h) against expectations derived from OracleMaxSum alone: the oracle is stepped one cycle at a
time, active(c) is the number of entries != 4 in count_v2f and count_f2v after cycle c, and t* is the first cycle c with
active(c - 1) == active(c) == 0 -- the first cycle that sent nothing.  The test functions live here;
tests/test_maxsum_quiescence_emu.py (emulated build) and tests/test_gpu_maxsum_quiescence.py (the HIP library) import them
and provide the `lib_path` fixture and the lists of parity cases, so the two runs cannot drift apart."""
import dataclasses
import functools

import numpy as np
import pytest

from parity_common import parity_cases
from pydcop_amd import generators as G
from pydcop_amd.dynamic import DynamicMaxSum
from pydcop_amd.engine import MaxSumEngine, MaxSumGpuError
from pydcop_amd.graph import Params

CAP = 300
STATE_KEYS = ("v2f", "f2v", "count_v2f", "count_f2v", "idx", "belief")
PARITY = {name: (make, kw) for name, make, kw in parity_cases()}
# the f32 subset: every family of the parity cases, those that end and those that never do
F32_CASES = ("coloring3_soft", "ising", "nary_meeting_d24", "nary_arity4_d5", "hard_nary_d8_i8_varcost_min",
             "box_i16_d24_two_passes", "bin2_peav_slots23", "bin2_coloring8_i8", "wide_hub_deg100", "hub_deg300",
             "hub_deg1100_max_all", "secp_small_m4_all", "multi_arity3_d64_float_all", "multi_arity6_mixed_dims")


@functools.lru_cache(maxsize=None)
def parity_graph(name):
    return PARITY[name][0]()


def parity_names(max_edges, subset=None):
    """the parity cases with at most `max_edges` edges (of `subset`), for a twin's pytest_generate_tests"""
    return [n for n in (subset or sorted(PARITY)) if parity_graph(n).n_edges <= max_edges]


def active_of(ora):
    _, _, cv, cf = ora.messages()
    return int((cv != 4).sum() + (cf != 4).sum())


def same_state(a, b, what=""):
    """element for element, as parity_common.compare_with_oracle compares an engine with the oracle (a NaN equals a NaN;
    max mode negates on the way out, so an engine's zero may be -0.0 where the oracle's is 0.0)"""
    for k in STATE_KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what} {k}")


def derive(graph, params, cap, beyond=0, change=None):
    """-> (active [cap' + 1] with active[0] = None, t* or None, the oracle's state() where it stopped); the oracle stops
    `beyond` cycles after t*, else at `cap`.  change = (cycle, factor, table): update_factor_table after that cycle,
    t* is then the first silent cycle after it."""
    from oracle.maxsum_oracle import OracleMaxSum
    ora = OracleMaxSum(graph, params, threads=8 if graph.n_edges > 2000 else 1)      # (the same bits, sooner)
    active, t_star, last = [None], None, -2
    for c in range(1, cap + 1):
        ora.run(1)
        active.append(active_of(ora))
        if active[c] == 0:
            if last == c - 1 and t_star is None:
                t_star = c
            last = c
        if change and change[0] == c:      # the fixed point no longer holds: detection starts again
            ora.update_factor_table(change[1], change[2])
            t_star, last = None, -2
        if t_star is not None and c >= t_star + beyond and not (change and c < change[0]):
            break
    state = ora.state()
    ora.close()
    return active, t_star, state


@functools.lru_cache(maxsize=None)
def expected(name, dtype="f64"):
    """a parity case: the instance, its parameters, t* within CAP and the oracle's state at t* (at CAP when there is
    none).  The oracle side checks the premise first: after the first silent cycle the state stays as it is."""
    graph, params = parity_graph(name), Params(**{**PARITY[name][1], "dtype": dtype})
    active, t_star, state = derive(graph, params, CAP)
    if t_star is not None:
        assert t_star >= 5
        _, again, later = derive(graph, params, CAP + 7, beyond=7)
        assert again == t_star and later["cycles"] == t_star + 7
        same_state(state, later, name)
    return graph, params, t_star, state, active


def q(active_at):
    """W -> the detection cycle, from the oracle's active(c) alone: the first checked c (c % W <= 1) with no active edge
    whose predecessor was checked with none either"""
    def at(W, cap):
        last = -2
        for c in range(1, cap + 1):
            if c % W <= 1 and active_at[c] == 0:
                if last == c - 1:
                    return c
                last = c
        return None
    return at


def watching(graph, params, every, lib_path, **pkw):
    eng = MaxSumEngine(graph, dataclasses.replace(params, **pkw), lib_path=lib_path)
    eng.watch_quiescence(every)
    return eng


def test_the_oracle_ends_on_most_parity_cases(oracle_built):
    """a condition, not a measurement: detection cannot pass by never detecting anything"""
    ends = [n for n in sorted(PARITY) if expected(n)[2] is not None]
    print(len(ends), "of", len(PARITY), "parity cases end within", CAP, "cycles (f64)")
    assert len(ends) >= 45
    for name, t in (("coloring3_soft", 87), ("nary_meeting_d24", 31), ("nary_arity4_d5", 9), ("hard_nary_d8_i8_varcost_min", 9),
                    ("box_i16_d24_two_passes", 46), ("bin2_peav_slots23", 88), ("wide_coloring6_deg30", 296),
                    ("hub_deg300", 107), ("hub_deg1100_max_all", 56), ("hub_scalefree_2000", 191), ("secp_small_m4_all", 24),
                    ("multi_arity3_d64_float_all", 45), ("multi_arity6_mixed_dims", 19), ("hard_nary_d24_i8_varcost", 30),
                    ("bin2_coloring8_hard_i16_max_all", 21), ("hard_box_overhang_varcost", 29),
                    ("hard_multi_arity3_d40_neg_inf", 38), ("ising", None), ("secp_small", None), ("hub_deg3400", None),
                    ("bin2_coloring8_i8", None)):
        assert expected(name)[2] == t, (name, expected(name)[2], t)


def check_detection(name, dtype, lib_path):
    graph, params, t_star, state, _ = expected(name, dtype)
    with watching(graph, params, 1, lib_path) as eng:
        r = eng.run_until_quiescent(CAP)
        qd = eng.quiescence()
        print(name, dtype, "engine", r, "oracle t*", t_star)
        assert r["quiescent"] == qd["quiescent"] == eng.quiescent == (t_star is not None)
        assert r["cycle"] == qd["cycle"] == t_star
        # spans of the default 64 cycles: stopped at the first span end at or after t*
        assert r["cycles_run"] == eng.cycle_count == (CAP if t_star is None else min(CAP, -(-t_star // 64) * 64))
        same_state(eng.state(), state, name)       # (after t* nothing changes: the oracle's state at t* is that of any later cycle)
    with MaxSumEngine(graph, params, lib_path=lib_path) as plain:
        plain.run(CAP)
        same_state(plain.state(), state, name)


def test_detection_equals_the_oracles_f64(case, lib_path, oracle_built):
    check_detection(case, "f64", lib_path)


def test_detection_equals_the_oracles_f32(f32_case, lib_path, oracle_built):
    check_detection(f32_case, "f32", lib_path)


_RC31N = lambda: G.random_coloring(60, seed=31)
ACTIVE_CASES = {"min": ({}, 64), "max": ({"mode": "max"}, 58), "start_all": ({"start_messages": "all"}, 62),
                "undamped": ({"damping_nodes": "none"}, 37), "tight": ({"stability": 1e-9}, 126)}


@functools.lru_cache(maxsize=None)
def rc31(variant="min"):
    graph, params = _RC31N(), Params(**ACTIVE_CASES[variant][0])
    active, t_star, _ = derive(graph, params, 200, beyond=10)
    assert t_star == ACTIVE_CASES[variant][1], (variant, t_star)
    return graph, params, active, t_star


@pytest.mark.parametrize("variant", sorted(ACTIVE_CASES))
def test_active_per_check(variant, lib_path, oracle_built):
    graph, params, active, t_star = rc31(variant)
    with watching(graph, params, 1, lib_path) as eng:
        assert eng.quiescence() == {"quiescent": False, "cycle": None, "checks": 0, "active": 0, "last_check_cycle": -1}
        for c in range(1, t_star + 4):
            eng.run(1)
            got = eng.quiescence()
            assert (got["active"], got["checks"], got["last_check_cycle"]) == (active[c], c, c), (c, got, active[c])
            assert got["quiescent"] == (c >= t_star) and got["cycle"] == (t_star if c >= t_star else None)


def drive(eng, how, cycles):
    if how == "one":
        eng.run(cycles)
    elif how == "steps":
        for _ in range(cycles):
            eng.run(1)
    elif how == "async13":
        left = cycles
        while left:
            eng.run_async(min(13, left))
            left -= min(13, left)
        eng.sync()
    elif how == "timed":
        eng.run_timed(cycles)
    else:
        eng.run_reps(cycles // 2, 2)


@pytest.mark.parametrize("every, at", [(4, 65), (7, 64), (2, 64), (16, 65)])
def test_wider_periods_replay_and_splitting(every, at, lib_path, oracle_built):
    """W = 4 detects at 65, W = 7 at 64 (64 % 7 == 1); W = 2 checks every cycle; W = 16 makes the default chunk one period"""
    graph, params, active, t_star = rc31()
    assert t_star == 64 and q(active)(every, 74) == at
    seen = []
    for chunk in (-1, 8, 0):
        for how in ("one", "steps", "async13", "timed", "reps"):
            with watching(graph, params, every, lib_path, graph_chunk=chunk) as eng:
                drive(eng, how, 120)
                seen.append(eng.quiescence())
    want = {"quiescent": True, "cycle": at, "checks": sum(1 for c in range(1, 121) if c % every <= 1), "active": 0,
            "last_check_cycle": max(c for c in range(1, 121) if c % every <= 1)}
    assert all(s == want for s in seen), (want, seen)
    for chunk in (-1, 8, 0):
        with watching(graph, params, every, lib_path, graph_chunk=chunk) as eng:
            r = eng.run_until_quiescent(200, poll=10)
            assert r == {"quiescent": True, "cycle": at, "cycles_run": 70} and eng.cycle_count == 70
            assert eng.run_until_quiescent(200, poll=10) == {"quiescent": True, "cycle": at, "cycles_run": 0}
            assert eng.cycle_count == 70
        with watching(graph, params, every, lib_path, graph_chunk=chunk) as eng:
            assert eng.run_until_quiescent(200, poll=1) == {"quiescent": True, "cycle": at, "cycles_run": at}
            assert eng.run_until_quiescent(200) == {"quiescent": True, "cycle": at, "cycles_run": 0}
        with watching(graph, params, every, lib_path, graph_chunk=chunk) as eng:      # the cap comes first
            assert eng.run_until_quiescent(50, poll=20) == {"quiescent": False, "cycle": None, "cycles_run": 50}


@pytest.mark.parametrize("name, make, end", [("ising", lambda: G.ising_grid(8, 8, seed=3), 428),
                                             ("scalefree", lambda: G.scalefree_coloring(100, seed=2, unary_noise=0), 610)])
def test_never_quiescent(name, make, end, lib_path, oracle_built):
    graph, params = make(), Params()
    active, t_star, state = derive(graph, params, 400)
    assert t_star is None and active[400] == end
    with watching(graph, params, 1, lib_path) as eng:
        r = eng.run_until_quiescent(400)
        assert r == {"quiescent": False, "cycle": None, "cycles_run": 400} and not eng.quiescent
        got = eng.quiescence()
        assert (got["active"], got["checks"], got["last_check_cycle"]) == (end, 400, 400)
        same_state(eng.state(), state, name)


def test_invalidation(lib_path, oracle_built):
    make = lambda: G.random_mixed(30, 65, seed=34, dom_choices=(2, 3, 4))
    graph, params = make(), Params()
    _, t_star, _ = derive(graph, params, 100)
    assert t_star == 29
    lo, hi = int(graph.table_off[0]), int(graph.table_off[1])
    first = graph.tables[lo:hi].copy()
    table = first[::-1] * 3.0 + 1.0
    _, t_new, s_new = derive(make(), params, 300, change=(40, 0, table))
    assert t_new is not None and t_new > 41, t_new
    graph = make()      # (update_factor_table keeps the host copy in step: not on an instance used above)
    with watching(graph, params, 1, lib_path) as eng:
        eng.run(10)
        at10 = eng.state()
        eng.run(30)
        assert eng.quiescent and eng.quiescence()["cycle"] == 29 and eng.cycle_count == 40
        eng.update_factor_table(0, table)
        got = eng.quiescence()
        assert not eng.quiescent and got["cycle"] is None and got["checks"] == 40      # (the checks are kept)
        r = eng.run_until_quiescent(300, poll=1)
        assert r == {"quiescent": True, "cycle": t_new, "cycles_run": t_new - 40}
        same_state(eng.state(), s_new)
        eng.update_factor_table(0, first)      # the first table again, and back to the state of cycle 10
        assert not eng.quiescent
        eng.set_state(**at10)
        assert not eng.quiescent and eng.cycle_count == 10
        assert eng.run_until_quiescent(300, poll=1) == {"quiescent": True, "cycle": 29, "cycles_run": 19}
        eng.set_state(**at10)                  # set_state on a quiescent engine
        assert not eng.quiescent
        eng.run(30)
        assert eng.quiescence()["cycle"] == 29
        eng.reset()
        assert not eng.quiescent and eng.cycle_count == 0
        eng.run(35)
        assert eng.quiescence()["cycle"] == 29


def anytime_snapshot(eng):
    b, (cyc, cost, viol, evals) = eng.best(), eng.cost_trace()
    return (b["cycle"], np.float64(b["cost"]).tobytes(), b["violations"], b["idx"].tobytes(), cyc.tobytes(), cost.tobytes(),
            viol.tobytes(), evals)


@pytest.mark.parametrize("track, every", [(1, 1), (4, 3), (5, 4)])
def test_together_with_track_best(track, every, lib_path, oracle_built):
    graph, params = G.random_coloring(60, seed=31, unary_noise=0), Params()
    active, t_star, _ = derive(graph, params, 100, beyond=10)
    assert t_star == 72
    at = q(active)(every, 82)
    for chunk in (-1, 8, 0):
        kw = {"graph_chunk": chunk}
        with MaxSumEngine(graph, dataclasses.replace(params, **kw), lib_path=lib_path) as alone:
            alone.track_best(track, float("inf"), 200)
            alone.run(100)
            tracked = anytime_snapshot(alone)
        with watching(graph, params, every, lib_path, **kw) as alone:
            alone.run(100)
            watched = alone.quiescence()
        assert watched["cycle"] == at
        for first in ("track", "watch"):
            with MaxSumEngine(graph, dataclasses.replace(params, **kw), lib_path=lib_path) as eng:
                if first == "watch":
                    eng.watch_quiescence(every)
                eng.track_best(track, float("inf"), 200)
                if first == "track":
                    eng.watch_quiescence(every)
                eng.run(100)
                assert anytime_snapshot(eng) == tracked and eng.quiescence() == watched, (chunk, first)


def test_refusals_change_nothing(lib_path, oracle_built):
    graph, params, _, _ = rc31()
    with MaxSumEngine(graph, params, lib_path=lib_path) as eng:
        for call in (eng.quiescence, lambda: eng.run_until_quiescent(10)):
            with pytest.raises(MaxSumGpuError, match="error -5"):      # before watch_quiescence
                call()
        with pytest.raises(MaxSumGpuError, match="error -1"):
            eng.watch_quiescence(-1)
        with pytest.raises(MaxSumGpuError, match="error -5"):          # ... which has not switched it on
            eng.quiescence()
        assert eng.quiescent is False and eng.cycle_count == 0
        eng.watch_quiescence(1)
        eng.run(5)
        before = eng.quiescence()
        with pytest.raises(MaxSumGpuError, match="error -1"):
            eng.watch_quiescence(-2)
        with pytest.raises(MaxSumGpuError, match="error -1"):
            eng.run_until_quiescent(-1)
        assert eng.cycle_count == 5 and eng.quiescence() == before


def test_debug_timeline_is_refused_while_watching(lib_path, oracle_built):
    graph, params, _, _ = rc31()
    with watching(graph, params, 1, lib_path) as eng:
        eng.run(5)
        before = eng.quiescence()
        with pytest.raises(MaxSumGpuError, match="error -5"):
            eng.debug_timeline()
        assert eng.cycle_count == 5 and eng.quiescence() == before


@pytest.mark.parametrize("step", ["step_compute", "step_pack", "step_unpack"])
def test_step_calls_are_refused_while_watching(step, lib_path, oracle_built):
    graph, params, _, _ = rc31()
    with watching(graph, params, 1, lib_path) as eng:
        eng.run(5)
        before = eng.quiescence()
        with pytest.raises(MaxSumGpuError, match="error -5"):
            getattr(eng, step)()
        assert eng.cycle_count == 5 and eng.quiescence() == before


def test_halo_setup_is_refused_while_watching(lib_path, oracle_built):
    graph, params, _, _ = rc31()
    with watching(graph, params, 1, lib_path) as eng:
        with pytest.raises(MaxSumGpuError, match="error -5"):
            eng.halo_setup(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
        eng.run(3)
        assert eng.quiescence()["checks"] == 3


def test_a_sharded_engine_is_refused(lib_path, oracle_built):
    graph, params, _, _ = rc31()
    with MaxSumEngine(graph, params, lib_path=lib_path) as eng:
        eng.halo_setup(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
        with pytest.raises(MaxSumGpuError, match="error -5"):
            eng.watch_quiescence(1)
        with pytest.raises(MaxSumGpuError, match="error -5"):
            eng.quiescence()


def test_lifecycle(lib_path, oracle_built):
    from oracle.maxsum_oracle import OracleMaxSum
    graph, params, active, t_star = rc31()
    ora = OracleMaxSum(graph, params)
    with MaxSumEngine(graph, params, lib_path=lib_path) as eng:
        assert eng.quiescent is False           # never switched on: the engine of before
        eng.run(40), ora.run(40)
        same_state(eng.state(), ora.state())
        assert eng.quiescent is False
        eng.watch_quiescence(3)                 # switched on in the middle of a run: the checks start with the next cycle
        eng.run(40)
        got = eng.quiescence()
        assert got == {"quiescent": True, "cycle": q(active)(3, 74), "checks": sum(1 for c in range(41, 81) if c % 3 <= 1),
                       "active": 0, "last_check_cycle": 79}
        eng.watch_quiescence(1)                 # again: starts again, on a state that is at rest already
        assert eng.quiescence() == {"quiescent": False, "cycle": None, "checks": 0, "active": 0, "last_check_cycle": -1}
        eng.run(2)
        assert eng.quiescence() == {"quiescent": True, "cycle": 82, "checks": 2, "active": 0, "last_check_cycle": 82}
        eng.watch_quiescence(0)                 # off: the buffers are gone
        assert eng.quiescent is False
        with pytest.raises(MaxSumGpuError, match="error -5"):
            eng.quiescence()
        eng.run(3), ora.run(43)
        same_state(eng.state(), ora.state())
    ora.close()


def test_dynamic_maxsum_forwards_and_a_scope_change_keeps_watching(lib_path, oracle_built):
    graph, params = G.random_mixed(30, 65, seed=34, dom_choices=(2, 3, 4)), Params()
    with DynamicMaxSum(graph, params, lib_path=lib_path) as run:
        assert run.quiescent is False
        run.watch_quiescence(1)
        assert run.run_until_quiescent(100, poll=1) == {"quiescent": True, "cycle": 29, "cycles_run": 29}
        assert run.quiescent and run.quiescence()["cycle"] == 29
        f = next(f for f in range(graph.n_factors) if graph.factor_rowptr[f + 1] - graph.factor_rowptr[f] == 2)
        a, b = (int(v) for v in graph.edge_var[graph.factor_rowptr[f]:graph.factor_rowptr[f] + 2])
        c = next(v for v in range(graph.n_vars) if v not in (a, b))
        table = np.arange(int(graph.dom_size[a]) * int(graph.dom_size[c]), dtype=np.float64)
        run.change_factor_function(f, table, scope=[a, c])      # a new engine: watching with the same period, not quiescent
        assert run.relayouts == 1 and not run.quiescent
        assert run.quiescence() == {"quiescent": False, "cycle": None, "checks": 0, "active": 0, "last_check_cycle": -1}
        run.run(2)
        assert run.quiescence()["checks"] == 2
