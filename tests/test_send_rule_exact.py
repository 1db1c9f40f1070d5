"""The send rule without the division (pydcop_amd/csrc/send_rule.h) decides exactly what the reference's
quotient decides.  tests/send_rule_check.cpp includes the header the kernels include and compares, for
double and float: a = 2 |prev - c| at 0, +-1 .. +-64 ulps around stability * s over the full exponent range
of s = |prev + c|; subnormal a and s; prev + c == 0 and prev == c; +-inf and NaN in either operand;
stability in {0, 2^-20, 0.1, 0.5, 1, 8}; and it fails if the fast path leaves more than 0.1 % of ordinary
random inputs to the division.  Built twice: plain, and with the address and undefined-behaviour sanitizers
(a stand-alone binary, nothing else in the process)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "send_rule_check.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "pydcop_amd", "csrc")]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_send_rule_equals_the_plain_quotient(sanitize, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "send_rule_check")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
             "-static-libasan", "-static-libubsan"] if sanitize else []  # (the runtimes inside the binary itself)
    subprocess.check_call([cxx] + FLAGS + extra + [SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("OK ")]
    assert [ln.split()[1] for ln in lines] == ["double", "float"], r.stdout
    assert not r.stderr.strip(), r.stderr[-2000:]  # (a sanitizer report)
