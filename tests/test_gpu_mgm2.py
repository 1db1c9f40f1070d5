"""MGM-2 on the GPU (pydcop_amd/csrc/mgm2.h through the mxs_mgm2_* C-ABI) against tests/mgm2_oracle.py
(pinned against the reference's own Mgm2Computation): values, held costs and has_cost bit for bit,
round by round, f64 and f32; a 100k-variable colouring and a 5k-variable meeting instance."""
import numpy as np
import pytest

from mgm2_common import compare_mgm2, mgm2_cases
from pydcop_amd import generators as G
from pydcop_amd.graph import Params

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", mgm2_cases(), ids=lambda c: c[0])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mgm2_bit_exact_vs_oracle(case, dtype):
    from mgm2_oracle import OracleMgm2
    name, make, pkw, kw = case
    compare_mgm2(OracleMgm2, make(), Params(dtype=dtype, **pkw), kw)


def _same_state(eng, ora, what):
    se, so = eng.state(), ora.state()
    for key in ("idx", "has_cost", "cost"):
        np.testing.assert_array_equal(se[key], so[key], err_msg=f"{key} {what}")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mgm2_100k_coloring(dtype):
    from mgm2_oracle import OracleMgm2
    from pydcop_amd.mgm2 import Mgm2Engine
    g = G.random_coloring(100_000, seed=0, names=False)
    p = Params(dtype=dtype)
    with Mgm2Engine(g, p, seed=9) as eng:
        ora = OracleMgm2(g, p, seed=9)
        start = eng.eval_cost()[0]
        for r in range(3):
            eng.run(1), ora.run(1)
            _same_state(eng, ora, f"after {r + 1} rounds")
        eng.run(40)
        assert eng.eval_cost()[0] < 0.6 * start


def test_mgm2_meeting_5k():
    from mgm2_oracle import OracleMgm2
    from pydcop_amd.mgm2 import Mgm2Engine
    g = G.meeting_like(5000, dom=24, arity=3, seed=3, names=False)
    p = Params(mode="max")
    with Mgm2Engine(g, p, favor="no", seed=4) as eng:
        ora = OracleMgm2(g, p, favor="no", seed=4)
        for r in range(2):
            eng.run(1), ora.run(1)
            _same_state(eng, ora, f"after {r + 1} rounds")


def test_mgm2_library_is_the_hip_build():
    from pydcop_amd.engine import MGM2_SYMBOLS, load_library
    lib = load_library()
    assert lib.mxs_build_kind() == 1 and lib.mxs_version() >= 230
    for name in MGM2_SYMBOLS:
        getattr(lib, name)


@pytest.mark.parametrize("path", __import__("mgm2_common").mgm2_golden_files(), ids=lambda p: p.rsplit("/", 1)[-1])
def test_mgm2_equals_the_reference_fixtures(path):
    """tests/golden/mgm2/: what the reference's own computations held after T rounds."""
    from mgm2_common import check_golden, load_mgm2_golden
    from pydcop_amd.mgm2 import Mgm2Engine
    g, pkw, kw, rounds, ref_idx, ref_cost = load_mgm2_golden(path)
    with Mgm2Engine(g, Params(**pkw), **kw) as e:
        e.run(rounds)
        check_golden(e.state(), ref_idx, ref_cost)
