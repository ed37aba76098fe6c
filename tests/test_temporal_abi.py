"""CPU-only: the clip entry points (ofmk_signature_rgb8, ofmk_signature_distances, ofmk_align_residuals_rgb8; build extensions) are
exported, declared and bound, and refuse bad arguments with OFMK_E_ARG before any HIP call, so this runs without a GPU (the pointer
values below are never dereferenced).  The ABI stays 6: the three calls are additions."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

E_ARG = -1
h, w, H, W, M, N, SPAN = 57, 91, 72, 104, 3, 5, 7
LIB, LEAK, FIRST, RES, SIG, DIST = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
SIG_NAME, DIST_NAME, RES_NAME = "ofmk_signature_rgb8", "ofmk_signature_distances", "ofmk_align_residuals_rgb8"
IDENTITY = (65536, 0, 0, 0, 65536, 0)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from offmark import _hip
    return _hip.load()


def refused(lib, rc):
    return rc == E_ARG and lib.ofmk_last_error().decode() != ""


def sig_refused(lib, inp=LEAK, n=M, fh=h, fw=w, sig=SIG, opts=None):
    return refused(lib, lib.ofmk_signature_rgb8(inp, n, fh, fw, sig, None, opts))


def dist_refused(lib, a=SIG, m=M, b=SIG + 0x1000, n=N, dist=DIST, opts=None):
    return refused(lib, lib.ofmk_signature_distances(a, m, b, n, dist, None, opts))


def res_refused(lib, library=LIB, n=N, leak=LEAK, m=M, lh=h, lw=w, ch=H, cw=W, first=FIRST, span=SPAN, geom=IDENTITY, res=RES, opts=None):
    from offmark import _hip
    g = None if geom is None else C.byref(_hip.Affine(*geom))
    return refused(lib, lib.ofmk_align_residuals_rgb8(library, n, leak, m, lh, lw, ch, cw, first, span, g, res, None, opts))


def test_the_symbols_are_exported_declared_and_bound(lib):
    from offmark import _hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "offmark_hip.h")).read(), flags=re.S)
    for name in (SIG_NAME, DIST_NAME, RES_NAME):
        assert hasattr(lib, name) and name in _hip.SIGNATURES and name in _hip.SYMBOLS
    tail = r"void\s*\*\s*stream\s*,\s*const\s+ofmk_opts\s*\*\s*opts\s*\)"
    assert re.search(r"\bint\s+" + SIG_NAME + r"\s*\(const\s+uint8_t\s*\*\s*in\s*,\s*int\s+n\s*,\s*int\s+h\s*,\s*int\s+w\s*,\s*uint8_t\s*\*\s*sig\s*,\s*" + tail, header)
    assert re.search(r"\bint\s+" + DIST_NAME + r"\s*\(const\s+uint8_t\s*\*\s*a\s*,\s*int\s+m\s*,\s*const\s+uint8_t\s*\*\s*b\s*,\s*int\s+N\s*,\s*int32_t\s*\*\s*dist\s*,\s*"
                     + tail, header)
    assert re.search(r"\bint\s+" + RES_NAME + r"\s*\(const\s+uint8_t\s*\*\s*lib\s*,\s*int\s+N\s*,\s*const\s+uint8_t\s*\*\s*leak\s*,\s*int\s+m\s*,\s*int\s+h\s*,\s*int\s+w\s*,\s*"
                     r"int\s+H\s*,\s*int\s+W\s*,\s*const\s+int32_t\s*\*\s*first\s*,\s*int\s+span\s*,\s*const\s+ofmk_affine\s*\*\s*geom\s*,\s*long\s+long\s*\*\s*res\s*,\s*"
                     + tail, header)
    assert lib.ofmk_version() == 6 == _hip.ABI_VERSION
    assert re.search(r"#define\s+OFMK_ABI_VERSION\s+6\b", header)


def test_the_bindings_argument_types(lib):
    from offmark import _hip
    vp, i32, op, ap = C.c_void_p, C.c_int, C.POINTER(_hip.Opts), C.POINTER(_hip.Affine)
    want = {SIG_NAME: [vp, i32, i32, i32, vp, vp, op], DIST_NAME: [vp, i32, vp, i32, vp, vp, op],
            RES_NAME: [vp, i32, vp, i32, i32, i32, i32, i32, vp, i32, ap, vp, vp, op]}
    for name, args in want.items():
        res, got = _hip.SIGNATURES[name]
        assert res is i32 and got == args
        fn = getattr(lib, name)
        assert fn.restype is i32 and list(fn.argtypes) == args


def bad_opts():
    from offmark import _hip
    return C.byref(_hip.Opts(1 << 20, 0, None)), C.byref(_hip.Opts(0, 65, None))


def test_signature_refuses_bad_arguments(lib):
    assert sig_refused(lib, inp=None) and sig_refused(lib, sig=None)
    assert sig_refused(lib, n=0) and sig_refused(lib, n=-3)
    assert sig_refused(lib, fh=7) and sig_refused(lib, fw=7) and sig_refused(lib, fh=0) and sig_refused(lib, fw=-8)      # a cell would be empty
    assert sig_refused(lib, fh=1 << 14, fw=1 << 14) and sig_refused(lib, fh=8, fw=1 << 25)                              # h * w < 2^28
    assert all(sig_refused(lib, opts=o) for o in bad_opts())


def test_distances_refuses_bad_arguments(lib):
    assert dist_refused(lib, a=None) and dist_refused(lib, b=None) and dist_refused(lib, dist=None)
    assert dist_refused(lib, m=0) and dist_refused(lib, n=0) and dist_refused(lib, m=-1) and dist_refused(lib, n=-1)
    assert dist_refused(lib, m=1 << 20, n=1 << 20)                                                                     # m * N < 2^40
    assert all(dist_refused(lib, opts=o) for o in bad_opts())


def test_residuals_refuses_null_pointers(lib):
    assert res_refused(lib, library=None) and res_refused(lib, leak=None) and res_refused(lib, first=None) and res_refused(lib, res=None)
    assert res_refused(lib, geom=None)


def test_residuals_refuses_bad_counts_sizes_and_geometries(lib):
    assert res_refused(lib, n=0) and res_refused(lib, m=0) and res_refused(lib, n=-1) and res_refused(lib, m=-1)
    assert res_refused(lib, span=0) and res_refused(lib, span=17) and res_refused(lib, span=-7)
    assert res_refused(lib, ch=7) and res_refused(lib, cw=7) and res_refused(lib, ch=4097) and res_refused(lib, cw=4097)
    assert res_refused(lib, lh=0) and res_refused(lib, lw=0) and res_refused(lib, lh=-8) and res_refused(lib, lh=1 << 14, lw=1 << 14)
    assert res_refused(lib, geom=(0, 0, 0, 0, 0, 0))                                         # singular
    assert res_refused(lib, geom=((1 << 20) + 1, 0, 0, 0, 65536, 0))                         # a coefficient beyond 2^20
    assert res_refused(lib, geom=(65536, 0, (1 << 48) + 1, 0, 65536, 0))                     # an offset beyond 2^48
    assert all(res_refused(lib, opts=o) for o in bad_opts())
