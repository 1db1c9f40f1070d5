"""MGM-2 on the emulated engine build (the very same mgm.hip / mgm2.h, g++ against the fake HIP runtime)
against tests/mgm2_oracle.py, bit for bit, round by round -- the CPU twin of tests/test_gpu_mgm2.py."""
import pytest

from mgm2_common import compare_mgm2, mgm2_cases
from pydcop_amd.graph import Params


@pytest.fixture(scope="module")
def emu_lib():
    from emu.build_emu import build
    return build()


@pytest.mark.parametrize("case", mgm2_cases(), ids=lambda c: c[0])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mgm2_emu_bit_exact_vs_oracle(case, dtype, emu_lib):
    from mgm2_oracle import OracleMgm2
    name, make, pkw, kw = case
    compare_mgm2(OracleMgm2, make(), Params(dtype=dtype, **pkw), kw, lib_path=emu_lib)


def test_mgm2_emu_refuses_bad_parameters_and_tables(emu_lib):
    import numpy as np
    from pydcop_amd import generators as G
    from pydcop_amd.engine import MaxSumGpuError
    from pydcop_amd.mgm2 import Mgm2Engine
    g = G.random_coloring(20, seed=1)
    with pytest.raises(ValueError, match="favor"):
        Mgm2Engine(g, Params(), favor="both", lib_path=emu_lib)
    with pytest.raises(ValueError, match="threshold"):
        Mgm2Engine(g, Params(), threshold=1.5, lib_path=emu_lib)
    g.tables = g.tables.copy()
    g.tables[3] = np.nan
    with pytest.raises(MaxSumGpuError, match="finite"):
        Mgm2Engine(g, Params(), lib_path=emu_lib)
    g.tables[3] = np.inf
    with pytest.raises(MaxSumGpuError, match="finite"):
        Mgm2Engine(g, Params(), lib_path=emu_lib)


def test_mgm2_emu_seed_changes_the_run(emu_lib):
    import numpy as np
    from pydcop_amd import generators as G
    from pydcop_amd.mgm2 import Mgm2Engine
    g = G.random_coloring(200, seed=5)
    a, b = Mgm2Engine(g, Params(), seed=1, lib_path=emu_lib), Mgm2Engine(g, Params(), seed=2, lib_path=emu_lib)
    a.run(3), b.run(3)
    assert (a.assignment()[0] != b.assignment()[0]).any()
    a.close(), b.close()


@pytest.mark.parametrize("path", __import__("mgm2_common").mgm2_golden_files(), ids=lambda p: p.rsplit("/", 1)[-1])
def test_mgm2_oracle_and_emu_equal_the_reference_fixtures(path, emu_lib):
    """tests/golden/mgm2/: what the reference's own computations held after T rounds (tools/make_golden_mgm2.py)."""
    from mgm2_common import check_golden, load_mgm2_golden
    from mgm2_oracle import OracleMgm2
    from pydcop_amd.mgm2 import Mgm2Engine
    g, pkw, kw, rounds, ref_idx, ref_cost = load_mgm2_golden(path)
    o = OracleMgm2(g, Params(**pkw), **kw)
    o.run(rounds)
    check_golden(o.state(), ref_idx, ref_cost)
    with Mgm2Engine(g, Params(**pkw), lib_path=emu_lib, **kw) as e:
        e.run(rounds)
        check_golden(e.state(), ref_idx, ref_cost)
