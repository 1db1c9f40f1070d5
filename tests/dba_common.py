"""DBA: the cases and the engine-vs-oracle comparison shared by the emulated (CPU) and the GPU tests."""
import glob
import json
import os

import numpy as np

from gdba_common import from_scopes, matched_pairs_binary, stars_paths_unaries, triples_arity3
from mgm_common import repeated_pairs_and_unaries, shuffled_names, with_init
from pydcop_amd import generators as G
from pydcop_amd.dba import DbaEngine

ROUNDS = 12
HERE = os.path.dirname(os.path.abspath(__file__))
STATE_KEYS = ("idx", "has_cost", "cost", "eval", "improve", "new", "counter", "consistent")


def emu_lib():
    """The emulated library; tests/emu/build_emu.py does not list dba.h among its dependencies, so it is rebuilt
    here when dba.h is newer."""
    from emu.build_emu import OUT, build
    dba_h = os.path.join(os.path.dirname(HERE), "pydcop_amd", "csrc", "dba.h")
    return build(force=os.path.exists(OUT) and os.path.getmtime(OUT) < os.path.getmtime(dba_h))


def scaled(g, factor=1000.0):
    """Integer tables x 1000: with `infinity: 1000` every non-zero entry is a violation, evals stay far below it;
    no variable costs (DBA does not look at them)."""
    g.tables = g.tables * factor
    g.var_cost = np.zeros_like(g.var_cost)
    return g


def rings_arity3_dom24(seed):
    """Twelve variables of 24 values, arity-3 constraints along two rings of six: the register path at bound 32.
    Periodic 0 / 1000 tables (a quarter of the entries violated)."""
    from pydcop_amd.generators import _finish
    rng = np.random.default_rng(seed)
    dom = np.full(12, 24, dtype=np.int32)
    scopes, tabs = [], []
    a, b, c = np.meshgrid(np.arange(24), np.arange(24), np.arange(24), indexing="ij")
    for ring in (0, 6):
        for i in range(6):
            scopes.append([ring + i, ring + (i + 1) % 6, ring + (i + 2) % 6])
            p, q, k = (int(x) for x in rng.integers(1, 5, 3))
            tabs.append(1000.0 * (((p * a + q * b + c + k) % 4) == 0).reshape(-1))
    rowptr = np.arange(0, 3 * len(scopes) + 1, 3, dtype=np.int32)
    toff = np.arange(0, (len(scopes) + 1) * 24 ** 3, 24 ** 3, dtype=np.int64)
    return _finish(dom, np.zeros(int(dom.sum())), rowptr, np.array(scopes, dtype=np.int32).reshape(-1), np.concatenate(tabs), toff)


BIG_DOMS = [33, 70, 5, 64, 65, 8, 32, 3, 9, 17, 70, 33]


def binary_big_domains(seed, density=0.85):
    """Binary constraints over domains around every word boundary (32 | 33, 64 | 65) and up to 70 values: rows of
    one, two and three words, the generic kernel."""
    rng = np.random.default_rng(seed)
    n = len(BIG_DOMS)
    scopes = [[i, (i + 1) % n] if i % 2 else [(i + 1) % n, i] for i in range(n)]
    scopes += [[0, 4], [1, 10], [3, 4], [6, 0], [7, 2], [11, 5], [8, 9], [9, 8]]
    g = from_scopes(BIG_DOMS, scopes, rng, 0, 2)
    g.tables = 1000.0 * (np.random.default_rng(seed + 1).random(g.tables.shape[0]) < density)
    return g


def dba_cases():
    """(name, graph factory, DBA kwargs).  Tables are 0 or multiples of 1000, `infinity` is 1000."""
    hard = lambda n, seed, **kw: G.random_coloring(n, seed=seed, variant="hard", unary_noise=0, **kw)   # noqa: E731
    return [
        ("hard_deg2_shuffled", lambda: shuffled_names(hard(30, 82, avg_degree=2), 82), dict(infinity=1000, max_distance=3, seed=1)),
        ("hard_deg4_init", lambda: with_init(hard(30, 86), 86), dict(infinity=1000, max_distance=50, seed=2)),
        ("hard_150_deg4", lambda: hard(150, 93), dict(infinity=1000, max_distance=2, seed=3)),
        ("stars_paths_unaries", lambda: scaled(stars_paths_unaries(83)), dict(infinity=1000, max_distance=3, seed=4)),
        ("matched_pairs_binary", lambda: scaled(matched_pairs_binary(92)), dict(infinity=1000, max_distance=3, seed=5)),
        ("triples_arity3_init", lambda: scaled(triples_arity3(84)), dict(infinity=1000, max_distance=50, seed=6)),
        ("repeated_pairs_unaries", lambda: scaled(repeated_pairs_and_unaries(30, 87)), dict(infinity=1000, max_distance=50, seed=7)),
        ("mixed_int_arity3", lambda: scaled(G.random_mixed(24, 36, seed=88, float_tables=False, unary_noise=0)),
         dict(infinity=1000, max_distance=50, seed=8)),
        ("rings_arity3_dom24", lambda: rings_arity3_dom24(94), dict(infinity=1000, max_distance=4, seed=9)),
        ("binary_big_domains", lambda: binary_big_domains(95), dict(infinity=1000, max_distance=50, seed=10)),
    ]


def count_violations(g, idx, infinity):
    """the constraints whose entry under the assignment is >= infinity"""
    n = 0
    for f in range(g.n_factors):
        lin = 0
        for e in range(g.factor_rowptr[f], g.factor_rowptr[f + 1]):
            lin = lin * int(g.dom_size[g.edge_var[e]]) + int(idx[g.edge_var[e]])
        n += bool(g.tables[int(g.table_off[f]) + lin] >= infinity)
    return n


def same_state(eng, ora, what=""):
    se, so = eng.state(), ora.state()
    for key in STATE_KEYS:
        np.testing.assert_array_equal(se[key], so[key], err_msg=f"{key} {what}")
    np.testing.assert_array_equal(eng.weights(), ora.weights(), err_msg=f"weights {what}")
    assert (eng.finished, eng.stop_round, eng.cycle_count) == (ora.finished, ora.stop_round, ora.cycle_count), what


def compare_dba(oracle_cls, graph, params, kw, lib_path=None, steps=(0, 1, 1, 3, 7)):
    """Round by round: values, held costs, evals, improvements, new values, counters, consistent flags, every weight,
    finished and stop_round; 1 + 1 + 3 rounds are the state after 5; reset starts again; run after a stop
    changes nothing."""
    eng = DbaEngine(graph, params, lib_path=lib_path, **kw)
    ora = oracle_cls(graph, params, **kw)
    assert eng.mask_bytes == ora.mask_bytes
    for n in steps:
        eng.run(n), ora.run(n)
        same_state(eng, ora, f"after {ora.cycle_count} rounds")
        ce, co = eng.eval_cost(), ora.eval_cost()
        assert ce[1] == co[1]
        assert (np.isnan(ce[0]) and np.isnan(co[0])) or abs(ce[0] - co[0]) <= 1e-9 * max(1.0, abs(co[0]))
    if ora.finished:
        before, wb = eng.state(), eng.weights()
        eng.run(3), ora.run(3)
        same_state(eng, ora, "run after the stop")
        for key, val in eng.state().items():
            np.testing.assert_array_equal(val, before[key], err_msg=f"{key}: run after the stop")
        np.testing.assert_array_equal(eng.weights(), wb)
    eng.reset(), ora.reset()
    assert eng.cycle_count == 0 and not eng.finished and eng.stop_round == 0
    same_state(eng, ora, "after reset")
    eng.run(5), ora.run(5)
    after5, w5 = eng.state(), eng.weights()
    same_state(eng, ora, "5 rounds after reset")
    eng.reset()
    for n in (1, 1, 3):
        eng.run(n)
    for key, val in eng.state().items():
        np.testing.assert_array_equal(val, after5[key], err_msg=f"{key}: 1 + 1 + 3 rounds against 5")
    np.testing.assert_array_equal(eng.weights(), w5)
    eng.close(), ora.close()


def dba_golden_files():
    return sorted(glob.glob(os.path.join(HERE, "golden", "dba", "*.npz")))


def load_dba_golden(path):
    """tools/make_golden_dba.py -> (FlatGraph, DBA kwargs, rounds, ref, info): ref holds what the reference's own
    computations held after `rounds` rounds or at their stop (the keys of `state()`, and `weights`), info =
    {"moves", "increases", "stop_round", "rounds", "violations"}."""
    from pydcop_amd.graph import FlatGraph
    z = np.load(path)
    meta = json.loads(bytes(z["meta"]).decode())
    g = FlatGraph(dom_size=z["dom_size"], var_cost=z["var_cost"], factor_rowptr=z["factor_rowptr"],
                  edge_var=z["edge_var"], table_off=z["table_off"], tables=z["tables"].astype(np.float64),
                  var_rowptr=z["var_rowptr"], var_edges=z["var_edges"],
                  init_idx=z["init_idx"] if "init_idx" in z.files else None)
    g.var_names = meta["var_names"]
    ref = {k: z["ref_" + k] for k in STATE_KEYS + ("weights",)}
    return g.validate(), meta["dba"], meta["rounds"], ref, meta["info"]


def check_golden(eng, ref, info):
    """`eng`: a DbaEngine or the oracle, after run(rounds) on the fixture's instance"""
    state = eng.state()
    for key in STATE_KEYS:
        np.testing.assert_array_equal(state[key], ref[key], err_msg=key)
    np.testing.assert_array_equal(eng.weights(), ref["weights"])
    assert eng.cycle_count == info["rounds"] and eng.stop_round == info["stop_round"]
    assert eng.finished == bool(info["stop_round"])
