"""CPU-only: the tone entry points (ofmk_histograms_rgb8, ofmk_tone_sums_rgb8, ofmk_apply_tone_rgb8; build extensions) are exported,
declared and bound, and refuse bad arguments with OFMK_E_ARG before any HIP call, so this runs without a GPU (the pointer values below
are never dereferenced).  The ABI stays 6: the three calls are additions."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

E_ARG = -1
h, w, H, W, N, K = 56, 90, 72, 104, 3, 2
SRC, LEAK, CANDS, SUMS, OUT, LUT, HIST = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000
HIST_NAME, SUMS_NAME, APPLY_NAME = "ofmk_histograms_rgb8", "ofmk_tone_sums_rgb8", "ofmk_apply_tone_rgb8"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from offmark import _hip
    return _hip.load()


def refused(lib, rc):
    return rc == E_ARG and lib.ofmk_last_error().decode() != ""


def hist_refused(lib, inp=LEAK, n=N, lh=h, lw=w, hist=HIST, opts=None):
    return refused(lib, lib.ofmk_histograms_rgb8(inp, n, lh, lw, hist, None, opts))


def sums_refused(lib, src=SRC, leak=LEAK, n=N, lh=h, lw=w, ch=H, cw=W, cands=CANDS, k=K, sums=SUMS, opts=None):
    return refused(lib, lib.ofmk_tone_sums_rgb8(src, leak, n, lh, lw, ch, cw, cands, k, sums, None, opts))


def apply_refused(lib, inp=LEAK, n=N, lh=h, lw=w, lut=LUT, out=OUT, opts=None):
    return refused(lib, lib.ofmk_apply_tone_rgb8(inp, n, lh, lw, lut, out, None, opts))


def test_the_symbols_are_exported_declared_and_bound(lib):
    from offmark import _hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "offmark_hip.h")).read(), flags=re.S)
    for name in (HIST_NAME, SUMS_NAME, APPLY_NAME):
        assert hasattr(lib, name) and name in _hip.SIGNATURES and name in _hip.SYMBOLS
    tail = r"void\s*\*\s*stream\s*,\s*const\s+ofmk_opts\s*\*\s*opts\s*\)"
    assert re.search(r"\bint\s+" + HIST_NAME + r"\s*\(const\s+uint8_t\s*\*\s*in\s*,\s*int\s+n\s*,\s*int\s+h\s*,\s*int\s+w\s*,\s*long\s+long\s*\*\s*hist\s*,\s*" + tail, header)
    assert re.search(r"\bint\s+" + SUMS_NAME + r"\s*\(const\s+uint8_t\s*\*\s*src\s*,\s*const\s+uint8_t\s*\*\s*leak\s*,\s*int\s+n\s*,\s*int\s+h\s*,\s*int\s+w\s*,\s*"
                     r"int\s+H\s*,\s*int\s+W\s*,\s*const\s+ofmk_affine\s*\*\s*cands\s*,\s*int\s+K\s*,\s*long\s+long\s*\*\s*sums\s*,\s*" + tail, header)
    assert re.search(r"\bint\s+" + APPLY_NAME + r"\s*\(const\s+uint8_t\s*\*\s*in\s*,\s*int\s+n\s*,\s*int\s+h\s*,\s*int\s+w\s*,\s*const\s+uint8_t\s*\*\s*lut\s*,\s*"
                     r"uint8_t\s*\*\s*out\s*,\s*" + tail, header)
    assert lib.ofmk_version() == 6 == _hip.ABI_VERSION
    assert re.search(r"#define\s+OFMK_ABI_VERSION\s+6\b", header)


def test_the_bindings_argument_types(lib):
    from offmark import _hip
    vp, i32, op = C.c_void_p, C.c_int, C.POINTER(_hip.Opts)
    want = {HIST_NAME: [vp, i32, i32, i32, vp, vp, op], SUMS_NAME: [vp, vp, i32, i32, i32, i32, i32, vp, i32, vp, vp, op],
            APPLY_NAME: [vp, i32, i32, i32, vp, vp, vp, op]}
    for name, args in want.items():
        res, got = _hip.SIGNATURES[name]
        assert res is i32 and got == args
        fn = getattr(lib, name)
        assert fn.restype is i32 and list(fn.argtypes) == args


def test_the_engine_and_the_decoders_have_the_methods():
    from offmark.engine import DctEngine
    from offmark.extract.dct_decoder import DctDecoder
    from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder
    for name in ("histograms", "tone_sums", "apply_tone"):
        assert callable(getattr(DctEngine, name))
        assert callable(getattr(DwtDctSvdDecoder, name + "_u8")) and not hasattr(DctDecoder, name + "_u8")


def test_histograms_refuses_bad_arguments(lib):
    assert hist_refused(lib, inp=None) and hist_refused(lib, hist=None)
    assert hist_refused(lib, n=0) and hist_refused(lib, n=-3)
    assert hist_refused(lib, lh=0) and hist_refused(lib, lw=0) and hist_refused(lib, lw=-1) and hist_refused(lib, lh=1 << 14, lw=1 << 14)      # h * w < 2^28
    from offmark import _hip
    assert hist_refused(lib, opts=C.byref(_hip.Opts(1 << 20, 0, None))) and hist_refused(lib, opts=C.byref(_hip.Opts(0, 65, None)))


def test_tone_sums_refuses_null_pointers(lib):
    assert sums_refused(lib, src=None) and sums_refused(lib, leak=None) and sums_refused(lib, cands=None) and sums_refused(lib, sums=None)


def test_tone_sums_refuses_bad_counts_and_sizes(lib):
    assert sums_refused(lib, n=0) and sums_refused(lib, n=-2) and sums_refused(lib, k=0) and sums_refused(lib, k=-1)
    assert sums_refused(lib, ch=4097) and sums_refused(lib, cw=4097) and sums_refused(lib, ch=8, cw=1 << 20)
    assert sums_refused(lib, ch=7) and sums_refused(lib, cw=7)
    assert sums_refused(lib, lh=0) and sums_refused(lib, lw=0) and sums_refused(lib, lh=-8) and sums_refused(lib, lh=1 << 14, lw=1 << 14)
    assert sums_refused(lib, n=1 << 20, k=1 << 20)                                                                 # n * K < 2^40
    from offmark import _hip
    assert sums_refused(lib, opts=C.byref(_hip.Opts(1 << 20, 0, None))) and sums_refused(lib, opts=C.byref(_hip.Opts(0, 65, None)))


def test_apply_tone_refuses_bad_arguments(lib):
    assert apply_refused(lib, inp=None) and apply_refused(lib, lut=None) and apply_refused(lib, out=None)
    assert apply_refused(lib, n=0) and apply_refused(lib, n=-1)
    assert apply_refused(lib, lh=0) and apply_refused(lib, lw=0) and apply_refused(lib, lh=1 << 14, lw=1 << 14)
    from offmark import _hip
    assert apply_refused(lib, opts=C.byref(_hip.Opts(1 << 20, 0, None)))
