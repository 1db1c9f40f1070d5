"""A slice of the random-instance sweep of tests/fuzz_common.py (emulated engine build against the
oracles, bit for bit): the Max-Sum sweep, asynchronous Max-Sum, DSA and MGM on domains 1..17, arities 1..4,
every mode / precision / start / damping choice; MGM-2, GDBA, DBA and DPOP on the instances of
`local_instance` / `dpop_instance` and on every constructed instance of tests/edge_shapes.py; the replica engines
(DSA, MGM with keyed draws, MGM-2: replicas, device costs, ranking) on those of `replica_instance`, GDBA and DBA as
replicas on those of `gdba_replica_instance` / `dba_replica_instance`; and what the
oracles alone must show over the seeds of tests/test_gpu_fuzz.py for that sweep to prove anything."""
import pytest

import dba_common
import edge_shapes
import fuzz_common
from fuzz_common import fuzz_maxsum, fuzz_others


@pytest.mark.parametrize("seed", range(200, 230))
def test_fuzz_maxsum_emu(seed, oracle_built):
    from emu.build_emu import build
    fuzz_maxsum(seed, build())


@pytest.mark.parametrize("seed", list(range(0, 60)) + list(range(200, 225)))  # (0..59: the seeds the GPU twin runs)
def test_fuzz_amaxsum_dsa_mgm_emu(seed, oracle_built):
    from emu.build_emu import build
    fuzz_others(seed, build())


@pytest.mark.parametrize("seed", range(0, 24))
def test_fuzz_maxsum_emu_wide_domains(seed, oracle_built, monkeypatch):
    """The same sweep over the domains of the round-5 kernels (up to 33 values: lane grids of 16 / 64 lanes, the lane-per-edge
    class of 5..8 values, box records that overhang their tables) with their layout switches among the random flags."""
    from emu.build_emu import build
    monkeypatch.setenv("FUZZ_DOMS", "big")
    fuzz_maxsum(seed, build())


@pytest.fixture(scope="module")
def emu_lib():
    return dba_common.emu_lib()


# (seeds past the GPU twin's: small and large halves of local_instance alternate)
@pytest.mark.parametrize("seed", range(100, 108))
def test_fuzz_mgm2_emu(seed, emu_lib, oracle_built):
    fuzz_common.fuzz_mgm2(seed, emu_lib)


@pytest.mark.parametrize("seed", range(100, 108))
def test_fuzz_gdba_emu(seed, emu_lib):
    fuzz_common.fuzz_gdba(seed, emu_lib)


@pytest.mark.parametrize("seed", range(100, 108))
def test_fuzz_dba_emu(seed, emu_lib):
    fuzz_common.fuzz_dba(seed, emu_lib)


@pytest.mark.parametrize("seed", range(100, 108))
def test_fuzz_dpop_emu(seed, emu_lib):
    fuzz_common.fuzz_dpop(seed, emu_lib)


@pytest.mark.parametrize("seed", range(0, 12))
def test_fuzz_replicas_emu(seed, emu_lib, oracle_built):
    fuzz_common.fuzz_replicas(seed, emu_lib)


@pytest.mark.parametrize("seed", range(0, 12))
def test_fuzz_gdba_replicas_emu(seed, emu_lib):
    fuzz_common.fuzz_gdba_replicas(seed, emu_lib)


@pytest.mark.parametrize("seed", range(0, 12))
def test_fuzz_dba_replicas_emu(seed, emu_lib):
    fuzz_common.fuzz_dba_replicas(seed, emu_lib)


@pytest.mark.parametrize("edge", edge_shapes.all_edges(), ids=lambda e: e[0])
def test_edge_shapes_emu(edge, emu_lib, oracle_built):
    edge[1](emu_lib)


def test_custom_trees_of_the_dpop_sweep_differ_from_the_built_in_ones():
    import numpy as np
    from pydcop_amd.dpop import build_pseudotree
    differ = 0
    for seed in range(3, 40, 4):
        g, _, tree, _ = fuzz_common.dpop_instance(seed)
        assert tree is not None
        fuzz_common.measure_tree(g, tree)
        differ += not np.array_equal(tree[0], build_pseudotree(g)[0])
    assert differ >= 8


# ---- the sweep must not pass vacuously: the oracles alone, over the seeds the GPU runs -------------------
@pytest.mark.parametrize("engine", sorted(fuzz_common.GPU_SEEDS))
def test_the_sweep_is_not_vacuous(engine, oracle_built):
    seeds = fuzz_common.GPU_SEEDS[engine]
    rows = [fuzz_common.oracle_summary(engine, s) for s in seeds]
    n = len(rows)
    if engine == "dba":
        idle = [s for s, r in zip(seeds, rows) if 0 < r["stop_round"] < 3 or r["increases"] == 0]
        failed = [s for s, r in zip(seeds, rows) if r["failed"]]
        equal_inf = [s for s, r in zip(seeds, rows) if r["kw"]["infinity"] == 2]
        print(f"dba: {len(idle)} of {n} seeds stop before round 3 or never raise a weight {idle}; "
              f"{len(failed)} end in the 'no best value' error {failed}; {len(equal_inf)} with infinity = 2")
        assert 4 * len(idle) <= n
        assert failed and len(failed) < len(equal_inf)      # both ends of the `infinity: 2` draws are met
    elif engine == "gdba":
        zero = [s for s, r in zip(seeds, rows) if r["pool"] == 0]
        print(f"gdba: {len(zero)} of {n} seeds end with an all-zero modifier pool {zero}")
        assert 4 * len(zero) <= n
        variants = {}
        for r in rows:
            k = (r["kw"]["modifier"], r["kw"]["violation"], r["kw"]["increase_mode"])
            pool, moves = variants.get(k, (0, 0))
            variants[k] = (pool + (r["pool"] > 0), moves + (r["moves"] > 0))
        assert len(variants) == 24
        assert all(pool > 0 and moves > 0 for pool, moves in variants.values()), variants
    elif engine == "mgm2":
        inner = [r for r in rows if 0 < r["kw"]["threshold"] < 1]
        moved = sum(r["pair_moves"] > 0 for r in inner)
        print(f"mgm2: {moved} of {len(inner)} seeds with 0 < threshold < 1 see a committed pair move")
        assert inner and 2 * moved >= len(inner)
    elif engine == "replicas":
        blocks = [s for s, r in zip(seeds, rows) if r["cost_blocks"] >= 2]
        init_blocks = [s for s, r in zip(seeds, rows) if r["n_vars"] > 256]
        many = [s for s, r in zip(seeds, rows) if r["replicas"] == 66]
        narrowed = [s for s, r in zip(seeds, rows) if r["f32_float_tables"]]
        apart = [s for s, r in zip(seeds, rows) if r["start_apart"] and r["end_apart"]]
        ambiguous = [s for s, r in zip(seeds, rows) if r["ambiguous_winner"]]
        print(f"replicas: {len(blocks)} of {n} seeds with two or more cost blocks {blocks}, {len(init_blocks)} over 256 "
              f"variables, {len(many)} with 66 replicas {many}, {len(narrowed)} in f32 on tables that are not f32-exact "
              f"{narrowed}, {len(apart)} whose replicas start apart and end apart, {len(ambiguous)} whose two best "
              f"reference costs lie within the bound of each other {ambiguous}")
        assert blocks and many and narrowed and apart
        assert len(init_blocks) == len([s for s in seeds if s % 3 == 2])
        assert any(s in blocks for s in many) and any(r["replicas"] > 1 for s, r in zip(seeds, rows) if s in blocks)
        assert 2 * len(apart) >= len([r for r in rows if r["replicas"] > 1])
        assert 10 * len(ambiguous) < n
        assert {r["replicas"] for r in rows} == set(fuzz_common.REPLICA_COUNTS)
    elif engine in ("gdba_replicas", "dba_replicas"):
        multi = [r for r in rows if r["replicas"] > 1]
        blocks = [s for s, r in zip(seeds, rows) if r["blocks"] >= 2 and r["replicas"] > 1]
        many = [s for s, r in zip(seeds, rows) if r["replicas"] == 66]
        apart = [s for s, r in zip(seeds, rows) if r["replicas"] > 1 and r["start_apart"] and r["end_apart"]]
        print(f"{engine}: {len(blocks)} of {n} seeds with two or more blocks of the reduction and R > 1 {blocks}, "
              f"{len(many)} with 66 replicas {many}, {len(apart)} of {len(multi)} with R > 1 whose replicas start apart "
              f"and end apart")
        assert blocks and many and 2 * len(apart) >= len(multi)
        assert len([s for s in seeds if rows[s - seeds[0]]["n_vars"] >= 260]) == len([s for s in seeds if s % 3 == 2])
        assert {r["replicas"] for r in rows} == set(fuzz_common.REPLICA_COUNTS)
        if engine == "dba_replicas":
            mixed = [s for s, r in zip(seeds, rows) if r["mixed_stops"]]
            mixed_each = [s for s, r in zip(seeds, rows) if r["mixed_stops"] and r["stop"] == "each"]
            failed = [s for s, r in zip(seeds, rows) if r["failed"]]
            print(f"dba_replicas: {len(mixed)} seeds whose replicas stop in different rounds or not at all {mixed} "
                  f"({len(mixed_each)} under stop='each'), {len(failed)} end early in the 'no best value' error {failed}")
            assert mixed and mixed_each
            assert {r["stop"] for r in rows if r["ended"]} == set(fuzz_common.DBA_STOPS)    # both policies end an engine
            assert failed and 3 * len(failed) <= n
    else:
        wide = sum(r["widest"] >= 2 for r in rows)
        ones = sum(r["one_value_in_separator"] for r in rows)
        shrinks = max(r["shrinks"] for r in rows)
        print(f"dpop: {wide} of {n} seeds with a separator of two or more variables, {ones} with a one-value variable "
              f"in a separator, at most {shrinks} shrink steps, {sum(r['shrinks'] > 0 for r in rows)} seeds shrunk")
        assert 2 * wide >= n and ones >= 5 and shrinks <= 2
