"""No DPOP kernel may use scratch (a per-thread array indexed at run time would): the compiler's resource
remarks for gfx950 (`make -C pydcop_amd/csrc resource-usage-mgm`), read here.  Compile only: no GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dpop_kernels_use_no_scratch():
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "pydcop_amd", "csrc"), "resource-usage-mgm"],
                         capture_output=True, text=True, check=True).stderr
    found, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and "k_dpop_" in name:
            found[name] = int(m.group(1))
    # util and value, each for (double | float) x (min | max)
    assert sum("k_dpop_util" in n for n in found) == 4 and sum("k_dpop_value" in n for n in found) == 4, sorted(found)
    assert all(s == 0 for s in found.values()), found
