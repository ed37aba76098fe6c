"""CPU-only: the colour entry points (ofmk_colour_sums_rgb8, ofmk_apply_colour_rgb8; build extensions) are exported, declared and
bound, and refuse bad arguments with OFMK_E_ARG before any HIP call, so this runs without a GPU (the device pointer values below are
never dereferenced; the matrix is HOST memory and is read).  The ABI stays 6: the two calls are additions."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

E_ARG = -1
h, w, H, W, N, K = 56, 90, 72, 104, 3, 2
SRC, LEAK, CANDS, SUMS, OUT = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
SUMS_NAME, APPLY_NAME = "ofmk_colour_sums_rgb8", "ofmk_apply_colour_rgb8"
ONE = 65536
IDENTITY = (ONE, 0, 0, 0, 0, ONE, 0, 0, 0, 0, ONE, 0)
MAX_COEFF, MAX_OFFSET = 1 << 21, 1 << 28


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from offmark import _hip
    return _hip.load()


def refused(lib, rc):
    return rc == E_ARG and lib.ofmk_last_error().decode() != ""


def sums_refused(lib, src=SRC, leak=LEAK, n=N, lh=h, lw=w, ch=H, cw=W, cands=CANDS, k=K, sums=SUMS, opts=None):
    return refused(lib, lib.ofmk_colour_sums_rgb8(src, leak, n, lh, lw, ch, cw, cands, k, sums, None, opts))


def matrix(values=IDENTITY):
    return (C.c_int32 * 12)(*values)


def apply_refused(lib, inp=LEAK, n=N, lh=h, lw=w, m=IDENTITY, out=OUT, opts=None):
    return refused(lib, lib.ofmk_apply_colour_rgb8(inp, n, lh, lw, None if m is None else matrix(m), out, None, opts))


def with_entry(i, v):
    m = list(IDENTITY)
    m[i] = v
    return m


def test_the_symbols_are_exported_declared_and_bound(lib):
    from offmark import _hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "offmark_hip.h")).read(), flags=re.S)
    for name in (SUMS_NAME, APPLY_NAME):
        assert hasattr(lib, name) and name in _hip.SIGNATURES and name in _hip.SYMBOLS
    tail = r"void\s*\*\s*stream\s*,\s*const\s+ofmk_opts\s*\*\s*opts\s*\)"
    assert re.search(r"\bint\s+" + SUMS_NAME + r"\s*\(const\s+uint8_t\s*\*\s*src\s*,\s*const\s+uint8_t\s*\*\s*leak\s*,\s*int\s+n\s*,\s*int\s+h\s*,\s*int\s+w\s*,\s*"
                     r"int\s+H\s*,\s*int\s+W\s*,\s*const\s+ofmk_affine\s*\*\s*cands\s*,\s*int\s+K\s*,\s*long\s+long\s*\*\s*sums\s*,\s*" + tail, header)
    assert re.search(r"\bint\s+" + APPLY_NAME + r"\s*\(const\s+uint8_t\s*\*\s*in\s*,\s*int\s+n\s*,\s*int\s+h\s*,\s*int\s+w\s*,\s*const\s+int32_t\s*\*\s*matrix\s*,\s*"
                     r"uint8_t\s*\*\s*out\s*,\s*" + tail, header)
    assert lib.ofmk_version() == 6 == _hip.ABI_VERSION
    assert re.search(r"#define\s+OFMK_ABI_VERSION\s+6\b", header)


def test_the_bindings_argument_types(lib):
    from offmark import _hip
    vp, i32, op, mp = C.c_void_p, C.c_int, C.POINTER(_hip.Opts), C.POINTER(C.c_int32)
    want = {SUMS_NAME: [vp, vp, i32, i32, i32, i32, i32, vp, i32, vp, vp, op], APPLY_NAME: [vp, i32, i32, i32, mp, vp, vp, op]}
    for name, args in want.items():
        res, got = _hip.SIGNATURES[name]
        assert res is i32 and got == args
        fn = getattr(lib, name)
        assert fn.restype is i32 and list(fn.argtypes) == args


def test_the_engine_and_the_decoders_have_the_methods():
    from offmark import colour
    from offmark.engine import DctEngine
    from offmark.extract.dct_decoder import DctDecoder
    from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder
    for name in ("colour_sums", "apply_colour"):
        assert callable(getattr(DctEngine, name))
        assert callable(getattr(DwtDctSvdDecoder, name + "_u8")) and not hasattr(DctDecoder, name + "_u8")
    for name in ("matrix_of_sums", "residual_rms", "read_coloured_leak"):
        assert callable(getattr(colour, name))


def test_colour_sums_refuses_null_pointers(lib):
    assert sums_refused(lib, src=None) and sums_refused(lib, leak=None) and sums_refused(lib, cands=None) and sums_refused(lib, sums=None)


def test_colour_sums_refuses_bad_counts_and_sizes(lib):
    assert sums_refused(lib, n=0) and sums_refused(lib, n=-2) and sums_refused(lib, k=0) and sums_refused(lib, k=-1)
    assert sums_refused(lib, ch=4097) and sums_refused(lib, cw=4097) and sums_refused(lib, ch=8, cw=1 << 20)
    assert sums_refused(lib, ch=7) and sums_refused(lib, cw=7)
    assert sums_refused(lib, lh=0) and sums_refused(lib, lw=0) and sums_refused(lib, lh=-8) and sums_refused(lib, lh=1 << 14, lw=1 << 14)
    assert sums_refused(lib, n=1 << 20, k=1 << 20)                                                                 # n * K < 2^40
    from offmark import _hip
    assert sums_refused(lib, opts=C.byref(_hip.Opts(1 << 20, 0, None))) and sums_refused(lib, opts=C.byref(_hip.Opts(0, 65, None)))


def test_apply_colour_refuses_bad_arguments(lib):
    assert apply_refused(lib, inp=None) and apply_refused(lib, m=None) and apply_refused(lib, out=None)
    assert apply_refused(lib, n=0) and apply_refused(lib, n=-1)
    assert apply_refused(lib, lh=0) and apply_refused(lib, lw=0) and apply_refused(lib, lh=1 << 14, lw=1 << 14)
    from offmark import _hip
    assert apply_refused(lib, opts=C.byref(_hip.Opts(1 << 20, 0, None)))


def test_apply_colour_refuses_a_matrix_out_of_range(lib):
    """|coefficient| <= 2^21 and |offset| <= 2^28 keep the sum inside int32; one past either, in any entry and either sign, is refused.
    (The limits themselves are accepted: that launches a kernel, so it is tested on the device, tests/test_gpu_colour.py.)"""
    for i in range(12):
        lim = MAX_OFFSET if i % 4 == 3 else MAX_COEFF
        assert apply_refused(lib, m=with_entry(i, lim + 1)) and apply_refused(lib, m=with_entry(i, -lim - 1)), i
    assert apply_refused(lib, m=with_entry(0, MAX_OFFSET))                       # an offset's size in a coefficient's place
    assert apply_refused(lib, m=with_entry(5, 2**31 - 1)) and apply_refused(lib, m=with_entry(7, -2**31))


def test_the_engine_refuses_a_bad_matrix_on_the_host():
    """DctEngine.apply_colour's own checks come after its check of the frames, which needs a device tensor; the shared range rule is
    offmark.colour.in_range, which matrix_of_sums uses to fall back to the identity."""
    import numpy as np
    from offmark import colour
    assert colour.in_range(colour.identity()) and colour.in_range(np.asarray(with_entry(3, MAX_OFFSET)).reshape(3, 4))
    assert colour.in_range(np.asarray(with_entry(0, -MAX_COEFF)).reshape(3, 4))
    assert not colour.in_range(np.asarray(with_entry(0, MAX_COEFF + 1)).reshape(3, 4))
    assert not colour.in_range(np.asarray(with_entry(11, -MAX_OFFSET - 1)).reshape(3, 4))
    assert not colour.in_range(np.zeros((4, 3), np.int32))
