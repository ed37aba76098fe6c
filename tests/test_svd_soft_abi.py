"""CPU-only: the soft read-out entry points (ofmk_svd_detect_soft_rgb8, ofmk_svd_detect_soft_yuv420, ofmk_detect_soft_yuv420; build
extensions, not reference semantics) are exported and refuse bad arguments with OFMK_E_ARG before any HIP call, as the matching
hard detect calls do, so these run without a GPU (the pointer values below are never dereferenced)."""
import ctypes as C

import pytest

E_ARG = -1
H, W, N, L = 64, 96, 3, 8
IN, SOFT, WS = 0x10000, 0x40000, 0x100000     # 8-byte (WS: 256-byte) aligned, never touched
SYMS = ("ofmk_svd_detect_soft_rgb8", "ofmk_svd_detect_soft_yuv420", "ofmk_detect_soft_yuv420")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from offmark import _hip
    return _hip.load()


def scales(*v):
    return (C.c_double * 3)(*v)


def call(lib, name, inp=IN, layout=0, n=N, h=H, w=W, sc=None, blk=4, l=L, soft=SOFT, opts=None):
    sc = scales(0, 15, 0) if sc is None else sc
    if name == "ofmk_svd_detect_soft_rgb8":
        return lib.ofmk_svd_detect_soft_rgb8(inp, n, h, w, l, sc, blk, soft, None, opts)
    if name == "ofmk_svd_detect_soft_yuv420":
        return lib.ofmk_svd_detect_soft_yuv420(inp, layout, n, h, w, l, sc, blk, soft, None, opts)
    return lib.ofmk_detect_soft_yuv420(inp, layout, n, h, w, l, 20.0, soft, 0, WS, 1 << 30, None, opts)


def test_symbols_are_exported_and_bound(lib):
    from offmark import _hip
    for name in SYMS:
        assert hasattr(lib, name) and name in _hip.SIGNATURES and name in _hip.SYMBOLS
    assert lib.ofmk_version() == 6


@pytest.mark.parametrize("name", SYMS)
def test_bad_arguments_return_e_arg_without_a_gpu(lib, name):
    svd, planar = name.startswith("ofmk_svd_"), name.endswith("_yuv420")
    assert call(lib, name, inp=None) == E_ARG
    assert call(lib, name, soft=None) == E_ARG
    assert call(lib, name, n=0) == E_ARG and call(lib, name, n=-3) == E_ARG
    assert call(lib, name, h=0) == E_ARG and call(lib, name, w=-8) == E_ARG and call(lib, name, h=4) == E_ARG
    assert call(lib, name, h=1 << 14, w=1 << 14) == E_ARG                        # H*W must be < 2^28
    assert call(lib, name, l=0) == E_ARG and call(lib, name, l=-1) == E_ARG
    if svd:
        assert call(lib, name, sc=C.cast(None, C.POINTER(C.c_double))) == E_ARG
        assert call(lib, name, blk=5) == E_ARG and call(lib, name, blk=2) == E_ARG and call(lib, name, blk=16) == E_ARG
        assert call(lib, name, sc=scales(0, float("nan"), 0)) == E_ARG
        assert call(lib, name, sc=scales(float("inf"), 15, 0)) == E_ARG
        assert call(lib, name, sc=scales(0, 1e-5, 0)) == E_ARG                   # a positive scale must be >= 1e-3 as float32
    if planar:
        assert call(lib, name, layout=2) == E_ARG and call(lib, name, layout=-1) == E_ARG
        assert call(lib, name, h=12) == E_ARG and call(lib, name, w=20) == E_ARG and call(lib, name, h=12, w=20) == E_ARG
        assert call(lib, name, inp=IN + 4) == E_ARG and call(lib, name, inp=IN + 1) == E_ARG
    assert "" != lib.ofmk_last_error().decode()


@pytest.mark.parametrize("name", SYMS)
def test_unknown_flag_bits_are_refused(lib, name):
    from offmark import _hip
    bad = _hip.Opts(1 << 20, 0, None)
    assert call(lib, name, opts=C.byref(bad)) == E_ARG
