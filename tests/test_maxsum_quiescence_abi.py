"""include/maxsum_gpu_quiescence.h: its declarations are engine.QUIESCENCE_SYMBOLS, the library exports them, the header
is C99, and a library without them is named in the error."""
import ctypes
import os
import re
import subprocess

import pytest

from pydcop_amd import generators as G
from pydcop_amd.engine import ABI_SYMBOLS, QUIESCENCE_SYMBOLS, MaxSumEngine, MaxSumGpuError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maxsum_gpu_quiescence.h")


def test_the_headers_symbols_are_the_bindings():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"\b(mxs_[a-z0-9_]+)\s*\(", text)
    assert tuple(declared) == QUIESCENCE_SYMBOLS
    assert not set(QUIESCENCE_SYMBOLS) & set(ABI_SYMBOLS)           # (a header of their own: not part of the pinned set)
    main = open(os.path.join(ROOT, "include", "maxsum_gpu.h")).read()
    assert not any(name in main for name in QUIESCENCE_SYMBOLS)


def test_the_emulated_library_exports_them():
    from emu.build_emu import build
    lib = ctypes.CDLL(build())
    for name in QUIESCENCE_SYMBOLS:
        assert getattr(lib, name) is not None


def test_the_header_is_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "maxsum_gpu_quiescence.h"\n'
                   "int use(mxs_engine *e) {\n"
                   "    int32_t q = 0; int64_t c = 0, n = 0, a = 0, l = 0, r = 0;\n"
                   "    int rc = mxs_watch_quiescence(e, 1);\n"
                   "    if (!rc) rc = mxs_run_until_quiescent(e, 100, 0, &q, &c, &r);\n"
                   "    if (!rc) rc = mxs_quiescence(e, &q, &c, &n, &a, &l);\n"
                   "    return rc ? rc : (int)(q + c + n + a + l + r);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "use.o")])


def test_a_library_without_the_symbols_is_named():
    from emu.build_emu import build
    with MaxSumEngine(G.random_coloring(20, seed=1), lib_path=build()) as eng:
        class Without:
            def __getattr__(self, name):
                if name in QUIESCENCE_SYMBOLS:
                    raise AttributeError(name)
                return getattr(real, name)
        real, eng._lib = eng._lib, Without()
        try:
            with pytest.raises(MaxSumGpuError, match="lacks mxs_watch_quiescence, mxs_quiescence, mxs_run_until_quiescent"):
                eng.watch_quiescence(1)
            assert eng.quiescent is False
        finally:
            eng._lib = real


def test_the_hip_library_exports_them():
    from pydcop_amd.engine import load_library
    lib = load_library()
    for name in QUIESCENCE_SYMBOLS:
        assert getattr(lib, name).restype is ctypes.c_int
