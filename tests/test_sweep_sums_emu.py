"""The neighbour sums of the packed variable classes (kernels.h, pack_sums: staged once in LDS, read in
chunks) in the emulated build: messages, counters, selection and beliefs bit for bit the oracle's after
every chunk of cycles, on instances whose degrees hit every boundary of the chunked loop."""
import pytest

from parity_common import compare_with_oracle
from pydcop_amd.graph import Params
from sweep_sums_cases import cases


@pytest.fixture(scope="session")
def emu_lib():
    from emu.build_emu import build
    return build()


@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_sweep_sums_emu(case, emu_lib, oracle_built):
    _, make, kw, steps, silent = case
    compare_with_oracle(oracle_built, make(), Params(**kw), 0, lib_path=emu_lib, exact=True, steps=steps,
                        expect_silent=silent)
