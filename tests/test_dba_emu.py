"""DBA on the emulated engine build (the very same mgm.hip / dba.h, g++ against the fake HIP runtime)
against tests/dba_oracle.py and the reference-recorded fixtures, value for value, round by round -- the
CPU twin of tests/test_gpu_dba.py."""
import numpy as np
import pytest

import dba_common
from dba_common import compare_dba, dba_cases
from pydcop_amd.graph import Params


@pytest.fixture(scope="module")
def emu_lib():
    return dba_common.emu_lib()


@pytest.mark.parametrize("case", dba_cases(), ids=lambda c: c[0])
def test_dba_emu_equals_oracle(case, emu_lib):
    from dba_oracle import OracleDba
    name, make, kw = case
    compare_dba(OracleDba, make(), Params(), kw, lib_path=emu_lib)


@pytest.mark.parametrize("path", dba_common.dba_golden_files(), ids=lambda p: p.rsplit("/", 1)[-1])
def test_dba_oracle_and_emu_equal_the_reference_fixtures(path, emu_lib):
    """tests/golden/dba/: what the reference's own computations held after T rounds or at their stop
    (tools/make_golden_dba.py)."""
    from dba_common import check_golden, count_violations, load_dba_golden
    from dba_oracle import OracleDba
    from pydcop_amd.dba import DbaEngine
    g, kw, rounds, ref, info = load_dba_golden(path)
    o = OracleDba(g, Params(), **kw)
    o.run(rounds)
    check_golden(o, ref, info)
    assert (o.moves, o.increases) == (info["moves"], info["increases"])
    assert count_violations(g, ref["idx"], kw["infinity"]) == info["violations"]
    with DbaEngine(g, Params(), lib_path=emu_lib, **kw) as e:
        e.run(rounds)
        check_golden(e, ref, info)


def test_dba_fixtures_move_increase_and_stop():
    """What the recorded cases must show for the suite to prove anything."""
    from dba_common import ROUNDS, load_dba_golden
    infos = [load_dba_golden(p)[4] for p in dba_common.dba_golden_files()]
    assert len(infos) == len(dba_cases())
    full = [i for i in infos if not i["stop_round"]]
    assert all(i["rounds"] == ROUNDS for i in full)
    assert sum(i["moves"] > 0 and i["increases"] > 0 for i in full) >= 4
    early = [i for i in infos if 0 < i["stop_round"] < ROUNDS]
    assert len(early) >= 3
    assert any(i["violations"] > 0 for i in early)
    assert all(i["moves"] > 0 for i in infos)


def test_dba_emu_refusals(emu_lib):
    from dba_common import scaled
    from dba_oracle import OracleDba
    from mgm_common import repeated_pairs_and_unaries
    from pydcop_amd import generators as G
    from pydcop_amd.dba import DbaEngine
    from pydcop_amd.engine import MaxSumGpuError
    g = G.random_coloring(20, seed=1, variant="hard", unary_noise=0)
    with pytest.raises(MaxSumGpuError, match="satisfaction"):
        DbaEngine(g, Params(mode="max"), lib_path=emu_lib)
    # the byte budget: the plan is sized before anything is allocated
    with DbaEngine(g, Params(), infinity=1000, lib_path=emu_lib) as e:
        need = e.mask_bytes
    assert need == 12 * len(g.var_edges)          # three rows of one word per slot
    with pytest.raises(MaxSumGpuError, match="budget"):
        DbaEngine(g, Params(), infinity=1000, mask_budget=1, lib_path=emu_lib)
    with pytest.raises(MaxSumGpuError, match="budget"):
        DbaEngine(g, Params(), infinity=1000, mask_budget=need - 1, lib_path=emu_lib)
    DbaEngine(g, Params(), infinity=1000, mask_budget=need, lib_path=emu_lib).close()
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(MaxSumGpuError, match="infinity must be finite"):
            DbaEngine(g, Params(), infinity=bad, lib_path=emu_lib)
    # weights and evals are int32: a round count that could overflow them is refused before anything runs
    with DbaEngine(g, Params(), infinity=1000, lib_path=emu_lib) as e:
        e.run(2)
        with pytest.raises(MaxSumGpuError, match="int32"):
            e.run(2 ** 31 - 1)
        assert e.cycle_count == 2
        e.run(1)
    # where the reference raises IndexError (every eval above infinity), run returns the error; so does the oracle
    h = scaled(repeated_pairs_and_unaries(30, 87))
    kw = dict(infinity=1, max_distance=50, seed=7)
    with DbaEngine(h, Params(), lib_path=emu_lib, **kw) as e:
        with pytest.raises(MaxSumGpuError, match="infinity"):
            e.run(3)
    with pytest.raises(IndexError):
        OracleDba(h, Params(), **kw).run(3)


def test_dba_emu_violation_bits_of_special_entries(emu_lib):
    """`entry >= infinity` in double: NaN is not violated, +inf is, an entry just below infinity is not."""
    from dba_oracle import OracleDba
    from pydcop_amd import generators as G
    g = G.random_coloring(40, seed=3, variant="hard", unary_noise=0)
    t = g.tables.copy()
    rng = np.random.default_rng(3)
    hot = np.flatnonzero(t >= 1000.0)
    t[hot[rng.random(hot.shape[0]) < 0.3]] = np.inf
    t[hot[rng.random(hot.shape[0]) < 0.2]] = np.nan
    t[hot[rng.random(hot.shape[0]) < 0.2]] = np.nextafter(1000.0, 0.0)
    g.tables = t
    compare_dba(OracleDba, g, Params(), dict(infinity=1000.0, max_distance=50, seed=4), lib_path=emu_lib)


def test_dba_emu_ignores_initial_values_and_seed_changes_the_run(emu_lib):
    from mgm_common import with_init
    from pydcop_amd import generators as G
    from pydcop_amd.dba import DbaEngine
    g = G.random_coloring(200, seed=5, variant="hard", unary_noise=0)
    a, b = DbaEngine(g, Params(), infinity=1000, seed=1, lib_path=emu_lib), DbaEngine(g, Params(), infinity=1000, seed=2, lib_path=emu_lib)
    start = a.assignment()[0].copy()
    a.run(3), b.run(3)
    assert (a.assignment()[0] != b.assignment()[0]).any()
    c = DbaEngine(with_init(g, 5), Params(), infinity=1000, seed=1, lib_path=emu_lib)   # dba.py:343 draws whatever the initial value
    np.testing.assert_array_equal(c.assignment()[0], start)
    a.close(), b.close(), c.close()
