"""The replica kernels of DBA (pydcop_amd/csrc/dba.h: k_dbar_*) use no scratch memory and come in the shapes of the
single run's -- the three register bounds, the wide walk, the decide phase -- plus the start state and the violation
count: hipcc's kernel-resource-usage remarks for gfx950 (`make -C pydcop_amd/csrc resource-usage-mgm`), read here.
Compile only: no GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"k_dbar_evalILi": 3, "k_dbar_eval_wide": 1, "k_dbar_decide": 1, "k_dbar_init": 1, "k_dbar_viol_partial": 1,
           "k_dbar_viol_final": 1}


def test_dba_replica_kernels_use_no_scratch():
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
    mine = {n: s for n, s in usage.items() if "k_dbar_" in n}
    for k, count in KERNELS.items():
        assert sum(k in n for n in mine) == count, (k, sorted(mine))
    assert len(mine) == sum(KERNELS.values()) and all(s == 0 for s in mine.values()), mine
    # the single run's entry points are still there beside them, the same five
    assert sum("k_dba_" in n for n in usage) == 5
