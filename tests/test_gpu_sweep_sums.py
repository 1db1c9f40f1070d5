"""The neighbour sums of the packed variable classes (kernels.h, pack_sums), the division-free send rule
(send_rule.h) and the min-instruction minima of the binary factors on the GPU: messages, counters,
selection and beliefs bit for bit the oracle's after every chunk of cycles, on the instances of
sweep_sums_cases.py (every boundary of the chunked loop, padding lanes, hard tables, silent edges,
the hub launch)."""
import pytest

from parity_common import compare_with_oracle
from pydcop_amd.graph import Params
from sweep_sums_cases import cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_gpu_sweep_sums(case, oracle_built):
    _, make, kw, steps, silent = case
    compare_with_oracle(oracle_built, make(), Params(**kw), 0, exact=True, steps=steps, expect_silent=silent)
