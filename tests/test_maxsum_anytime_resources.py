"""The kernels of Max-Sum's best-state tracking (pydcop_amd/csrc/anytime.h) use no scratch memory: hipcc's
kernel-resource-usage remarks for gfx950, read here.  The header is compiled in a unit of its own that launches both
kernels (engine.hip includes the very same header; compiling that takes minutes).  Compile only: no GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pydcop_amd", "csrc")
UNIT = """#include "anytime.h"
void launch_both(mxs::AnyState* st, mxs::AnyTrace tr, const double* pc, const unsigned long long* pv, const int32_t* sel,
                 int32_t* snap, hipStream_t s) {
    hipLaunchKernelGGL(mxs::k_any_final, dim3(1), dim3(mxs::ANY_TPB), 0, s, 1, 0, pc, pv, -1LL, 1, st, tr);
    hipLaunchKernelGGL(mxs::k_any_copy, dim3(1), dim3(mxs::ANY_TPB), 0, s, 1, sel, snap, st);
}
"""


def test_anytime_kernels_use_no_scratch(tmp_path):
    src = tmp_path / "anytime_unit.hip"
    src.write_text(UNIT)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", CSRC,
                        "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", os.devnull],
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
    mine = {n: s for n, s in usage.items() if "k_any_" in n}
    assert sum("k_any_final" in n for n in mine) == 1 and sum("k_any_copy" in n for n in mine) == 1, sorted(usage)
    assert all(s == 0 for s in mine.values()), mine
