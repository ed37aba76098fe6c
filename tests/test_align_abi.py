"""CPU-only: the registration entry points (ofmk_align_sums_rgb8, ofmk_halve_rgb8; build extensions) are exported, declared and
bound, and refuse bad arguments with OFMK_E_ARG before any HIP call, so this runs without a GPU (the pointer values below are never
dereferenced).  The ABI stays 6: both calls are additions."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

E_ARG = -1
h, w, H, W, N, K = 57, 91, 72, 104, 3, 2
SRC, LEAK, CANDS, SUMS, OUT = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
SUMS_NAME, HALVE_NAME = "ofmk_align_sums_rgb8", "ofmk_halve_rgb8"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from offmark import _hip
    return _hip.load()


def sums_refused(lib, src=SRC, leak=LEAK, n=N, lh=h, lw=w, ch=H, cw=W, cands=CANDS, k=K, sums=SUMS, opts=None):
    rc = lib.ofmk_align_sums_rgb8(src, leak, n, lh, lw, ch, cw, cands, k, sums, None, opts)
    return rc == E_ARG and lib.ofmk_last_error().decode() != ""


def halve_refused(lib, inp=LEAK, n=N, lh=h, lw=w, out=OUT, opts=None):
    rc = lib.ofmk_halve_rgb8(inp, n, lh, lw, out, None, opts)
    return rc == E_ARG and lib.ofmk_last_error().decode() != ""


def test_the_symbols_are_exported_declared_and_bound(lib):
    from offmark import _hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "offmark_hip.h")).read(), flags=re.S)
    for name in (SUMS_NAME, HALVE_NAME):
        assert hasattr(lib, name) and name in _hip.SIGNATURES and name in _hip.SYMBOLS
    assert re.search(r"\bint\s+" + SUMS_NAME + r"\s*\(const\s+uint8_t\s*\*\s*src\s*,\s*const\s+uint8_t\s*\*\s*leak\s*,\s*int\s+n\s*,\s*int\s+h\s*,\s*int\s+w\s*,\s*"
                     r"int\s+H\s*,\s*int\s+W\s*,\s*const\s+ofmk_affine\s*\*\s*cands\s*,\s*int\s+K\s*,\s*long\s+long\s*\*\s*sums\s*,\s*void\s*\*\s*stream\s*,\s*"
                     r"const\s+ofmk_opts\s*\*\s*opts\s*\)", header)
    assert re.search(r"\bint\s+" + HALVE_NAME + r"\s*\(const\s+uint8_t\s*\*\s*in\s*,\s*int\s+n\s*,\s*int\s+h\s*,\s*int\s+w\s*,\s*uint8_t\s*\*\s*out\s*,\s*"
                     r"void\s*\*\s*stream\s*,\s*const\s+ofmk_opts\s*\*\s*opts\s*\)", header)
    assert lib.ofmk_version() == 6 == _hip.ABI_VERSION
    assert re.search(r"#define\s+OFMK_ABI_VERSION\s+6\b", header)


def test_the_bindings_argument_types(lib):
    from offmark import _hip
    vp, i32, op = C.c_void_p, C.c_int, C.POINTER(_hip.Opts)
    want = {SUMS_NAME: [vp, vp, i32, i32, i32, i32, i32, vp, i32, vp, vp, op], HALVE_NAME: [vp, i32, i32, i32, vp, vp, op]}
    for name, args in want.items():
        res, got = _hip.SIGNATURES[name]
        assert res is i32 and got == args
        fn = getattr(lib, name)
        assert fn.restype is i32 and list(fn.argtypes) == args


def test_align_sums_refuses_null_pointers(lib):
    assert sums_refused(lib, src=None) and sums_refused(lib, leak=None) and sums_refused(lib, cands=None) and sums_refused(lib, sums=None)


def test_align_sums_refuses_bad_counts_and_sizes(lib):
    assert sums_refused(lib, n=0) and sums_refused(lib, n=-2) and sums_refused(lib, k=0) and sums_refused(lib, k=-1)
    assert sums_refused(lib, ch=4097) and sums_refused(lib, cw=4097) and sums_refused(lib, ch=8, cw=1 << 20)      # the int64 bound: H, W <= 4096
    assert sums_refused(lib, ch=7) and sums_refused(lib, cw=7)
    assert sums_refused(lib, lh=0) and sums_refused(lib, lw=0) and sums_refused(lib, lh=-8) and sums_refused(lib, lh=1 << 14, lw=1 << 14)
    assert sums_refused(lib, n=1 << 20, k=1 << 20)                                                                 # n * K < 2^40
    from offmark import _hip
    assert sums_refused(lib, opts=C.byref(_hip.Opts(1 << 20, 0, None))) and sums_refused(lib, opts=C.byref(_hip.Opts(0, 65, None)))


def test_halve_refuses_bad_arguments(lib):
    assert halve_refused(lib, inp=None) and halve_refused(lib, out=None)
    assert halve_refused(lib, n=0) and halve_refused(lib, n=-1)
    assert halve_refused(lib, lh=15) and halve_refused(lib, lw=15) and halve_refused(lib, lh=8, lw=8) and halve_refused(lib, lh=0)      # a halved side below 8
    assert halve_refused(lib, lh=1 << 14, lw=1 << 14)
    from offmark import _hip
    assert halve_refused(lib, opts=C.byref(_hip.Opts(1 << 20, 0, None)))
