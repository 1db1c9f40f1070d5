"""The random-instance sweep of tests/fuzz_common.py on the GPU: every engine of the library (the Max-Sum
sweep, asynchronous Max-Sum, DSA, MGM, MGM-2, GDBA, DBA, DPOP) against its oracle, bit for bit, on
instances nobody picked (domains 1..17, arities 1..4, every mode / precision / start / damping choice,
random layout flags; for the four newer engines up to 200 variables, unequal neighbour domains up to 65
values and every algorithm parameter; DSA, MGM with keyed draws, MGM-2, GDBA and DBA as 1..66 replicas of one
engine on up to 520 variables, with their device costs or violation counts and their ranking, DBA under both stop
policies), and the constructed edge instances of tests/edge_shapes.py."""
import pytest

import edge_shapes
import fuzz_common
from fuzz_common import fuzz_maxsum, fuzz_others

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", range(0, 80))
def test_fuzz_maxsum(seed, oracle_built):
    fuzz_maxsum(seed, None)


@pytest.mark.parametrize("seed", range(0, 60))
def test_fuzz_amaxsum_dsa_mgm(seed, oracle_built):
    fuzz_others(seed, None)


@pytest.mark.parametrize("seed", range(0, 40))
def test_fuzz_maxsum_wide_domains(seed, oracle_built, monkeypatch):
    """Domains up to 33 values (round 5: lane-grid factor kernels, the lane-per-edge variable class of 5..8 values, box records
    overhanging their tables), their layout switches among the random flags."""
    monkeypatch.setenv("FUZZ_DOMS", "big")
    fuzz_maxsum(seed, None)


@pytest.mark.parametrize("seed", fuzz_common.GPU_SEEDS["mgm2"])
def test_fuzz_mgm2(seed, oracle_built):
    fuzz_common.fuzz_mgm2(seed, None)


@pytest.mark.parametrize("seed", fuzz_common.GPU_SEEDS["gdba"])
def test_fuzz_gdba(seed):
    fuzz_common.fuzz_gdba(seed, None)


@pytest.mark.parametrize("seed", fuzz_common.GPU_SEEDS["dba"])
def test_fuzz_dba(seed):
    fuzz_common.fuzz_dba(seed, None)


@pytest.mark.parametrize("seed", fuzz_common.GPU_SEEDS["dpop"])
def test_fuzz_dpop(seed):
    fuzz_common.fuzz_dpop(seed, None)


@pytest.mark.parametrize("seed", fuzz_common.GPU_SEEDS["replicas"])
def test_fuzz_replicas(seed, oracle_built):
    fuzz_common.fuzz_replicas(seed, None)


@pytest.mark.parametrize("seed", fuzz_common.GPU_SEEDS["gdba_replicas"])
def test_fuzz_gdba_replicas(seed):
    fuzz_common.fuzz_gdba_replicas(seed, None)


@pytest.mark.parametrize("seed", fuzz_common.GPU_SEEDS["dba_replicas"])
def test_fuzz_dba_replicas(seed):
    fuzz_common.fuzz_dba_replicas(seed, None)


@pytest.mark.parametrize("edge", edge_shapes.all_edges(), ids=lambda e: e[0])
def test_edge_shapes(edge, oracle_built):
    edge[1](None)
