"""The single-run engines of MGM-2 and GDBA on the emulated engine build (the very same mgm2.h and gdba.h, g++ against
the fake HIP runtime): the CPU twin of tests/test_gpu_single_run.py.  The tests are those of tests/single_run_common.py."""
import pytest

from single_run_common import (  # noqa: F401  (collected here)
    test_reset_gives_the_fresh_state_and_the_same_run,
    test_the_start_states_have_the_shapes_the_cases_claim,
    test_single_run_equals_the_one_replica_engine,
    test_a_single_run_keeps_its_refusals)


@pytest.fixture(scope="module")
def lib_path():
    from emu.build_emu import build
    return build()
