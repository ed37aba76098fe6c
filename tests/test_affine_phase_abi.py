"""CPU-only: the dense shift search's entry point (ofmk_svd_affine_phase_scores_rgb8; a build extension) is exported, declared and
bound, and refuses bad arguments with OFMK_E_ARG before any HIP call, so this runs without a GPU (the pointer values below are never
dereferenced).  The ABI stays 6: the call is an addition."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

E_ARG = -1
h, w, H, W, N, K = 57, 91, 72, 104, 3, 6
IN, OUT, CANDS, UNITS = 0x10000, 0x20000, 0x30000, 0x40000
NAME = "ofmk_svd_affine_phase_scores_rgb8"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from offmark import _hip
    return _hip.load()


def scales(*v):
    return (C.c_double * 3)(*v)


def refused(lib, inp=IN, n=N, lh=h, lw=w, ch=H, cw=W, cands=CANDS, k=K, sc=None, blk=4, out=OUT, units=UNITS, opts=None):
    sc = scales(0, 15, 0) if sc is None else sc
    rc = lib.ofmk_svd_affine_phase_scores_rgb8(inp, n, lh, lw, ch, cw, cands, k, sc, blk, out, units, None, opts)
    return rc == E_ARG and lib.ofmk_last_error().decode() != ""


def test_the_symbol_is_exported_declared_and_bound(lib):
    from offmark import _hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "offmark_hip.h")).read(), flags=re.S)
    assert hasattr(lib, NAME) and NAME in _hip.SIGNATURES and NAME in _hip.SYMBOLS
    assert re.search(r"\bint\s+" + NAME + r"\s*\(const\s+uint8_t\s*\*\s*in\s*,\s*int\s+n\s*,\s*int\s+h\s*,\s*int\s+w\s*,\s*int\s+H\s*,\s*int\s+W\s*,\s*"
                     r"const\s+ofmk_affine\s*\*\s*cands\s*,\s*int\s+K\s*,\s*const\s+double\s*\*\s*scales\s*,\s*int\s+blk\s*,\s*long\s+long\s*\*\s*scores\s*,\s*"
                     r"long\s+long\s*\*\s*units\s*,\s*void\s*\*\s*stream\s*,\s*const\s+ofmk_opts\s*\*\s*opts\s*\)", header)
    assert lib.ofmk_version() == 6 == _hip.ABI_VERSION
    assert re.search(r"#define\s+OFMK_ABI_VERSION\s+6\b", header)


def test_the_bindings_argument_types(lib):
    from offmark import _hip
    res, args = _hip.SIGNATURES[NAME]
    vp, i32 = C.c_void_p, C.c_int
    assert res is i32
    assert args == [vp, i32, i32, i32, i32, i32, vp, i32, C.POINTER(C.c_double), i32, vp, vp, vp, C.POINTER(_hip.Opts)]
    fn = getattr(lib, NAME)
    assert fn.restype is i32 and list(fn.argtypes) == args
    # the scores-only sibling with one more pointer (units) in front of the stream
    sib = _hip.SIGNATURES["ofmk_svd_affine_scores_rgb8"][1]
    assert args[:11] == sib[:11] and args[12:] == sib[11:]


def test_null_pointers_are_refused_except_units(lib):
    assert refused(lib, inp=None) and refused(lib, out=None) and refused(lib, cands=None)
    assert refused(lib, sc=C.cast(None, C.POINTER(C.c_double)))
    # units may be NULL: with nothing else wrong the call gets past its argument checks (to HIP, which this machine may lack), so
    # the only thing to show here is that a NULL units does not change which bad arguments are refused
    assert refused(lib, units=None, n=0) and refused(lib, units=None, blk=8) and refused(lib, units=None, inp=None)


def test_counts_sizes_and_the_block_size(lib):
    assert refused(lib, n=0) and refused(lib, n=-2) and refused(lib, k=0) and refused(lib, k=-1)
    assert refused(lib, blk=8) and refused(lib, blk=5) and refused(lib, blk=0)
    assert refused(lib, lh=0) and refused(lib, lw=0) and refused(lib, lh=-8) and refused(lib, lh=1 << 14, lw=1 << 14)      # the leak: h * w < 2^28
    assert refused(lib, ch=7) and refused(lib, cw=7) and refused(lib, ch=1 << 14, cw=1 << 14)   # the canvas holds a unit and H * W < 2^28
    assert refused(lib, n=1 << 20, k=1 << 20)                                                  # n * K < 2^40


def test_scales_and_flags(lib):
    from offmark import _hip
    assert refused(lib, sc=scales(0, float("nan"), 0)) and refused(lib, sc=scales(float("inf"), 15, 0)) and refused(lib, sc=scales(0, 1e-4, 0))
    assert refused(lib, sc=scales(0, 0, 0)) and refused(lib, sc=scales(10, 0, 20)) and refused(lib, sc=scales(0, -15, 0))      # the search reads channel 1
    assert refused(lib, opts=C.byref(_hip.Opts(1 << 20, 0, None)))                     # unknown flag bits
    assert refused(lib, opts=C.byref(_hip.Opts(0, 65, None)))
