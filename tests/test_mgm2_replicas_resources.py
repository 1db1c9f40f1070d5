"""The replica kernels of MGM-2 (pydcop_amd/csrc/mgm2.h: k_mgm2r_*) use no scratch memory and come in exactly two
instantiations each (f32, f64): hipcc's kernel-resource-usage remarks for gfx950
(`make -C pydcop_amd/csrc resource-usage-mgm`), read here.  Compile only: no GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_mgm2r_init", "k_mgm2r_value", "k_mgm2r_offers", "k_mgm2r_receive", "k_mgm2r_resolve", "k_mgm2r_decide")


def test_mgm2_replica_kernels_use_no_scratch():
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
    mine = {n: s for n, s in usage.items() if any(k in n for k in KERNELS)}
    for k in KERNELS:   # f32 and f64 instantiations of each
        assert sum(k in n for n in mine) == 2, (k, sorted(mine))
    assert all(s == 0 for s in mine.values()), mine
    # the cost reduction is replica_cost.h's, instantiated for MGM-2's argument: no copy of it here
    cost = [n for n in usage if "k_cost_partial" in n and "mgm2" in n]
    assert len(cost) == 2 and all(usage[n] == 0 for n in cost), cost
