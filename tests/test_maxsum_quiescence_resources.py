"""The kernels of Max-Sum's quiescence check (pydcop_amd/csrc/quiescence.h) use no scratch memory: hipcc's
kernel-resource-usage remarks for gfx950, read here.  The header is compiled in a unit of its own that launches the
kernels (engine.hip includes the very same header; compiling that takes minutes).  Compile only: no GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pydcop_amd", "csrc")
UNIT = """#include "quiescence.h"
void launch_all(mxs::QuietLists ql, const uint8_t* cF, const uint8_t* cV, const double* f64, const float* f32, uint32_t* part,
                mxs::QuietState* st, hipStream_t s) {
    hipLaunchKernelGGL(mxs::k_quiet_count<double>, dim3(1), dim3(mxs::QUIET_TPB), 0, s, ql, cF, cV, f64, f64, part);
    hipLaunchKernelGGL(mxs::k_quiet_count<float>, dim3(1), dim3(mxs::QUIET_TPB), 0, s, ql, cF, cV, f32, f32, part);
    hipLaunchKernelGGL(mxs::k_quiet_final, dim3(1), dim3(mxs::QUIET_TPB), 0, s, 1, (const uint32_t*)part, 1, st);
    hipLaunchKernelGGL(mxs::k_quiet_restart, dim3(1), dim3(1), 0, s, st, 0LL, 1, 1);
}
"""


def test_quiescence_kernels_use_no_scratch(tmp_path):
    src = tmp_path / "quiescence_unit.hip"
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
    mine = {n: s for n, s in usage.items() if "k_quiet_" in n}
    assert sum("k_quiet_count" in n for n in mine) == 2 and sum("k_quiet_final" in n for n in mine) == 1, sorted(usage)
    assert all(s == 0 for s in mine.values()), mine
