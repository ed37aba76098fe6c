"""CPU-only: the toned-clip entry points (ofmk_align_moments_rgb8, ofmk_signature_ranks; build extensions) are exported, declared and
bound, and refuse bad arguments with OFMK_E_ARG before any HIP call, so this runs without a GPU (the pointer values below are never
dereferenced).  ofmk_align_moments_rgb8 has ofmk_align_residuals_rgb8's rules.  The ABI stays 6: the two calls are additions."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

E_ARG = -1
h, w, H, W, M, N, SPAN = 57, 91, 72, 104, 3, 5, 7
LIB, LEAK, FIRST, MOM, SIG, RANK = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
MOM_NAME, RANK_NAME = "ofmk_align_moments_rgb8", "ofmk_signature_ranks"
IDENTITY = (65536, 0, 0, 0, 65536, 0)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from offmark import _hip
    return _hip.load()


def refused(lib, rc):
    return rc == E_ARG and lib.ofmk_last_error().decode() != ""


def mom_refused(lib, library=LIB, n=N, leak=LEAK, m=M, lh=h, lw=w, ch=H, cw=W, first=FIRST, span=SPAN, geom=IDENTITY, mom=MOM, opts=None):
    from offmark import _hip
    g = None if geom is None else C.byref(_hip.Affine(*geom))
    return refused(lib, lib.ofmk_align_moments_rgb8(library, n, leak, m, lh, lw, ch, cw, first, span, g, mom, None, opts))


def rank_refused(lib, sig=SIG, n=N, rank=RANK, opts=None):
    return refused(lib, lib.ofmk_signature_ranks(sig, n, rank, None, opts))


def test_the_symbols_are_exported_declared_and_bound(lib):
    from offmark import _hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "offmark_hip.h")).read(), flags=re.S)
    for name in (MOM_NAME, RANK_NAME):
        assert hasattr(lib, name) and name in _hip.SIGNATURES and name in _hip.SYMBOLS
    tail = r"void\s*\*\s*stream\s*,\s*const\s+ofmk_opts\s*\*\s*opts\s*\)"
    assert re.search(r"\bint\s+" + MOM_NAME + r"\s*\(const\s+uint8_t\s*\*\s*lib\s*,\s*int\s+N\s*,\s*const\s+uint8_t\s*\*\s*leak\s*,\s*int\s+m\s*,\s*int\s+h\s*,\s*int\s+w\s*,\s*"
                     r"int\s+H\s*,\s*int\s+W\s*,\s*const\s+int32_t\s*\*\s*first\s*,\s*int\s+span\s*,\s*const\s+ofmk_affine\s*\*\s*geom\s*,\s*long\s+long\s*\*\s*mom\s*,\s*"
                     + tail, header)
    assert re.search(r"\bint\s+" + RANK_NAME + r"\s*\(const\s+uint8_t\s*\*\s*sig\s*,\s*int\s+n\s*,\s*uint8_t\s*\*\s*rank\s*,\s*" + tail, header)
    assert lib.ofmk_version() == 6 == _hip.ABI_VERSION
    assert re.search(r"#define\s+OFMK_ABI_VERSION\s+6\b", header)


def test_the_bindings_argument_types(lib):
    from offmark import _hip
    vp, i32, op, ap = C.c_void_p, C.c_int, C.POINTER(_hip.Opts), C.POINTER(_hip.Affine)
    want = {MOM_NAME: [vp, i32, vp, i32, i32, i32, i32, i32, vp, i32, ap, vp, vp, op], RANK_NAME: [vp, i32, vp, vp, op]}
    assert _hip.SIGNATURES[MOM_NAME] == _hip.SIGNATURES["ofmk_align_residuals_rgb8"]
    for name, args in want.items():
        res, got = _hip.SIGNATURES[name]
        assert res is i32 and got == args
        fn = getattr(lib, name)
        assert fn.restype is i32 and list(fn.argtypes) == args


def test_the_engine_and_the_decoder_carry_the_calls():
    from offmark.engine import DctEngine
    from offmark.extract.dct_decoder import DctDecoder
    from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder
    assert callable(DctEngine.align_moments) and callable(DctEngine.signature_ranks)
    assert callable(DwtDctSvdDecoder.align_moments_u8) and callable(DwtDctSvdDecoder.signature_ranks_u8)
    assert not hasattr(DctDecoder, "align_moments_u8") and not hasattr(DctDecoder, "signature_ranks_u8")


def bad_opts():
    from offmark import _hip
    return C.byref(_hip.Opts(1 << 20, 0, None)), C.byref(_hip.Opts(0, 65, None))


def test_ranks_refuses_bad_arguments(lib):
    assert rank_refused(lib, sig=None) and rank_refused(lib, rank=None)
    assert rank_refused(lib, n=0) and rank_refused(lib, n=-3)
    assert all(rank_refused(lib, opts=o) for o in bad_opts())


def test_moments_refuses_null_pointers(lib):
    assert mom_refused(lib, library=None) and mom_refused(lib, leak=None) and mom_refused(lib, first=None) and mom_refused(lib, mom=None)
    assert mom_refused(lib, geom=None)


def test_moments_refuses_bad_counts_sizes_and_geometries(lib):
    assert mom_refused(lib, n=0) and mom_refused(lib, m=0) and mom_refused(lib, n=-1) and mom_refused(lib, m=-1)
    assert mom_refused(lib, span=0) and mom_refused(lib, span=17) and mom_refused(lib, span=-7)
    assert mom_refused(lib, ch=7) and mom_refused(lib, cw=7) and mom_refused(lib, ch=4097) and mom_refused(lib, cw=4097)
    assert mom_refused(lib, lh=0) and mom_refused(lib, lw=0) and mom_refused(lib, lh=-8) and mom_refused(lib, lh=1 << 14, lw=1 << 14)
    assert mom_refused(lib, geom=(0, 0, 0, 0, 0, 0))                                         # singular
    assert mom_refused(lib, geom=((1 << 20) + 1, 0, 0, 0, 65536, 0))                         # a coefficient beyond 2^20
    assert mom_refused(lib, geom=(65536, 0, (1 << 48) + 1, 0, 65536, 0))                     # an offset beyond 2^48
    assert all(mom_refused(lib, opts=o) for o in bad_opts())
