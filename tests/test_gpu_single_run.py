"""The single-run engines of MGM-2 and GDBA on the GPU (pydcop_amd/csrc/mgm2.h, gdba.h through mxs_mgm2_create and
mxs_gdba_create): reset() against the fresh engine, the single run against the one-replica engine of the same seed,
the refusals a single run keeps.  The tests are those of tests/single_run_common.py; tests/test_single_run_emu.py is
the CPU twin."""
import pytest

from single_run_common import (  # noqa: F401  (collected here)
    test_reset_gives_the_fresh_state_and_the_same_run,
    test_single_run_equals_the_one_replica_engine,
    test_a_single_run_keeps_its_refusals)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib_path():
    return None
