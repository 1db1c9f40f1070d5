"""DBA on the GPU (pydcop_amd/csrc/dba.h through the mxs_dba_* C-ABI) against tests/dba_oracle.py (pinned
against the reference's own DbaComputation) and the reference-recorded fixtures of tests/golden/dba/: values,
held costs, evals, improvements, new values, counters, consistent flags, every weight and the stop round, round
by round."""
import numpy as np
import pytest

import dba_common
from dba_common import check_golden, compare_dba, load_dba_golden
from pydcop_amd.graph import Params

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("path", dba_common.dba_golden_files(), ids=lambda p: p.rsplit("/", 1)[-1])
def test_dba_equals_the_reference_fixtures_and_the_oracle(path):
    from dba_oracle import OracleDba
    from pydcop_amd.dba import DbaEngine
    g, kw, rounds, ref, info = load_dba_golden(path)
    with DbaEngine(g, Params(), **kw) as e:
        e.run(rounds)
        check_golden(e, ref, info)
    compare_dba(OracleDba, g, Params(), kw)


def test_dba_fixtures_are_all_there():
    assert len(dba_common.dba_golden_files()) == 10


def test_dba_refusals():
    from pydcop_amd.dba import DbaEngine
    from pydcop_amd.engine import MaxSumGpuError
    g = load_dba_golden(dba_common.dba_golden_files()[0])[0]
    with pytest.raises(MaxSumGpuError, match="satisfaction"):
        DbaEngine(g, Params(mode="max"))
    with pytest.raises(MaxSumGpuError, match="budget"):
        DbaEngine(g, Params(), infinity=1000, mask_budget=1)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(MaxSumGpuError, match="infinity must be finite"):
            DbaEngine(g, Params(), infinity=bad)


def test_dba_library_is_the_hip_build():
    from pydcop_amd.engine import ABI_SYMBOLS, load_library
    lib = load_library()
    assert lib.mxs_build_kind() == 1 and lib.mxs_version() >= 260
    for name in ABI_SYMBOLS:
        if name.startswith("mxs_dba_"):
            getattr(lib, name)
    assert sum(n.startswith("mxs_dba_") for n in ABI_SYMBOLS) == 10
