"""Instances for the neighbour sums of the packed variable classes (kernels.h, pack_sums): shared by
test_sweep_sums_emu.py (emulated build, CPU) and test_gpu_sweep_sums.py (HIP on the GPU).

A packed wave holds floor(64 / deg) variables of one degree side by side, one lane per edge, and
sums a variable's records in chunks of MXS_SUM_CHUNK neighbours plus an unrolled rest.  The
degrees below hit every boundary of that loop for a chunk of 4 and of 8: 1, 2, C - 1, C, C + 1, 2C,
2C + 1, then 15, 16, 17, 21 (three variables a wave, one padding lane), 32, 63 and 64 (a variable a
wave, one padding lane / none)."""
import numpy as np

from pydcop_amd import generators as G

CHUNKS = (4, 8)
DEGREES = sorted({1, 2, 15, 16, 17, 21, 32, 63, 64} | {d for c in CHUNKS for d in (c - 1, c, c + 1, 2 * c, 2 * c + 1)})


def degree_graph(degrees, n_colors, seed, copies=2, pool=None, variant="soft"):
    """`copies` centre variables of every degree in `degrees`, each tied by binary factors to that
    many DISTINCT variables drawn from a pool of leaves -- which thereby get small random degrees
    of their own (0 .. a handful), so a degree class is a mix of centres and leaves, its waves
    carry padding lanes, and consecutive waves of a class differ in degree."""
    rng = np.random.default_rng(seed)
    centres = [d for d in degrees for _ in range(copies)]
    pool = pool or max(degrees) + 16
    n = len(centres) + pool
    pairs = [(i, len(centres) + int(leaf)) for i, d in enumerate(centres) for leaf in rng.choice(pool, size=d, replace=False)]
    return G.random_coloring(n, n_colors=n_colors, seed=seed, variant=variant, pairs=np.array(pairs, dtype=np.int64), rng=rng)


def star(deg, n_colors, seed):
    """One centre of degree `deg` and its `deg` leaves of degree 1."""
    pairs = np.array([(0, 1 + i) for i in range(deg)], dtype=np.int64)
    return G.random_coloring(deg + 1, n_colors=n_colors, seed=seed, pairs=pairs)


def with_hard_entries(g, seed):
    """+-inf and NaN in the tables and +inf among the variables' own costs (dcop.py:352-365): the sums
    carry inf - inf = NaN, which -0.0 terms must leave as they are."""
    rng = np.random.default_rng(seed)
    t = g.tables.copy()
    u = rng.random(t.shape[0])
    t[u < 0.06] = np.inf
    t[(u >= 0.06) & (u < 0.09)] = -np.inf
    t[(u >= 0.09) & (u < 0.10)] = np.nan
    g.tables = t
    c = g.var_cost.copy()
    c[rng.random(c.shape[0]) < 0.03] = np.inf
    g.var_cost = c
    return g


def cases():
    """(id, graph factory, Params kwargs, steps, expect_silent)"""
    out = []
    # every degree boundary, D = 2, 3, 4 x f64 / f32, the modes and start modes spread over them
    spread = {2: [("min", "leafs"), ("max", "all")], 3: [("min", "leafs_vars"), ("max", "leafs")], 4: [("max", "leafs_vars"), ("min", "all")]}
    for D, combos in spread.items():
        for dtype, (mode, start) in zip(("f64", "f32"), combos):
            out.append((f"degrees_d{D}_{dtype}_{mode}_{start}", lambda D=D: degree_graph(DEGREES, D, seed=10 + D),
                        dict(dtype=dtype, mode=mode, start_messages=start), [0, 1, 1, 2, 6], False))
    # the three start modes on one instance (cycle 0 is the start cycle)
    for start in ("leafs", "leafs_vars", "all"):
        out.append((f"degrees_d3_start_{start}", lambda: degree_graph(DEGREES, 3, seed=3, copies=1),
                    dict(start_messages=start), [0, 1, 3], False))
    # stars: a wave of ONE variable and nothing else in its class
    for deg in (1, 5, 9, 21, 63, 64):
        out.append((f"star_{deg}", lambda deg=deg: star(deg, 3, seed=deg), dict(), [0, 1, 4], False))
    # random graphs of a few hundred variables, denser than the metric's (degrees up to ~20)
    out.append(("random_deg8_d3", lambda: G.random_coloring(300, avg_degree=8, seed=5), dict(), [1, 7], False))
    out.append(("random_deg8_d3_f32_max", lambda: G.random_coloring(300, avg_degree=8, seed=5), dict(dtype="f32", mode="max"), [1, 7], False))
    out.append(("random_deg12_d4_max", lambda: G.random_coloring(200, avg_degree=12, n_colors=4, seed=6), dict(mode="max"), [1, 7], False))
    out.append(("random_deg6_d2_f32", lambda: G.random_coloring(400, avg_degree=6, n_colors=2, seed=7), dict(dtype="f32"), [1, 7], False))
    # hard tables: +-inf and NaN entries
    out.append(("degrees_d3_hard_entries", lambda: with_hard_entries(degree_graph(DEGREES, 3, seed=8), 8), dict(), [0, 1, 2, 6], False))
    out.append(("degrees_d3_hard_entries_f32_max", lambda: with_hard_entries(degree_graph(DEGREES, 3, seed=8), 9),
                dict(dtype="f32", mode="max"), [0, 1, 2, 6], False))
    # long enough that send counters reach SAME_COUNT and edges fall silent
    out.append(("degrees_d3_silent", lambda: degree_graph(DEGREES, 3, seed=11, variant="hard"), dict(), [1, 39], True))
    # scale-free, ~2 000 variables: hub variables beyond degree 64 (k_sweep_hub) beside its packed classes
    out.append(("scalefree_2000", lambda: G.scalefree_coloring(2000, m=2, seed=12), dict(), [0, 1, 9], False))
    out.append(("scalefree_2000_f32_max", lambda: G.scalefree_coloring(2000, m=2, seed=12), dict(dtype="f32", mode="max"), [1, 5], False))
    return out
