"""The replica kernels of GDBA (pydcop_amd/csrc/gdba.h: k_gdbar_*) use no scratch memory and come in exactly the
expected instantiations -- f32 and f64 of the init, eval and decide kernels; the best-state copy kernel is the one
repcost::k_best_copy of the unit: hipcc's kernel-resource-usage remarks for gfx950
(`make -C pydcop_amd/csrc resource-usage-mgm`), read here.  Compile only: no GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"k_gdbar_init": 2, "k_gdbar_eval": 2, "k_gdbar_decide": 2}


def test_gdba_replica_kernels_use_no_scratch():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "pydcop_amd", "csrc"), "resource-usage-mgm"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            usage[name] = int(m.group(1))
    mine = {n: s for n, s in usage.items() if "k_gdbar_" in n}
    for k, count in KERNELS.items():
        assert sum(k in n for n in mine) == count, (k, sorted(mine))
    assert len(mine) == sum(KERNELS.values()), sorted(mine)
    assert all(s == 0 for s in mine.values()), mine
    # the snapshot of the best state is replica_cost.h's copy kernel: one in the unit, none of GDBA's own
    copy = [n for n in usage if "best_copy" in n]
    assert len(copy) == 1 and "k_best_copy" in copy[0] and usage[copy[0]] == 0, copy
    # the single-run kernels are still there, on the plain argument
    assert sum("k_gdba_eval" in n or "k_gdba_decide" in n for n in usage) == 4
    # the cost reduction is replica_cost.h's, instantiated for GDBA's argument: no copy of it here
    cost = [n for n in usage if "k_cost_partial" in n and "gdba" in n]
    assert len(cost) == 2 and all(usage[n] == 0 for n in cost), cost
