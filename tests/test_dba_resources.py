"""The DBA kernels (pydcop_amd/csrc/dba.h) use no scratch memory: hipcc's kernel-resource-usage
remarks for gfx950 (`make -C pydcop_amd/csrc resource-usage-mgm`), read here.  Compile only: no GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"k_dba_evalILi": 3, "k_dba_eval_wide": 1, "k_dba_decide": 1}   # the three register bounds, the generic one


def test_dba_kernels_use_no_scratch():
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
    mine = {n: s for n, s in usage.items() if "k_dba_" in n}
    for k, count in KERNELS.items():
        assert sum(k in n for n in mine) == count, (k, sorted(mine))
    assert len(mine) == sum(KERNELS.values()) and all(s == 0 for s in mine.values()), mine
