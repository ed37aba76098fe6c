"""CPU-only: the DwtDctSvd planar 4:2:0 entry points (ofmk_svd_*_yuv420) are exported and refuse bad arguments with
OFMK_E_ARG before any HIP call, so these run without a GPU (the pointer values below are never dereferenced)."""
import ctypes as C

import pytest

E_ARG = -1
H, W, N, L = 64, 96, 3, 8
IN, OUT, WM, CNT, BITS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000     # 8-byte aligned, never touched
SYMS = ("ofmk_svd_embed_yuv420", "ofmk_svd_detect_yuv420", "ofmk_svd_embed_detect_yuv420")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from offmark import _hip
    return _hip.load()


def scales(*v):
    return (C.c_double * 3)(*v)


def call(lib, name, inp=IN, out=OUT, layout=0, n=N, h=H, w=W, sc=None, blk=4, l=L, counts=CNT, bits=BITS, opts=None):
    sc = scales(0, 15, 0) if sc is None else sc
    if name == "ofmk_svd_embed_yuv420":
        return lib.ofmk_svd_embed_yuv420(inp, out, layout, n, h, w, WM, 1, None, sc, blk, None, opts)
    if name == "ofmk_svd_detect_yuv420":
        return lib.ofmk_svd_detect_yuv420(inp, layout, n, h, w, l, sc, blk, counts, bits, None, opts)
    return lib.ofmk_svd_embed_detect_yuv420(inp, out, layout, n, h, w, WM, 1, None, sc, blk, l, counts, bits, None, opts)


def test_symbols_are_exported_and_bound(lib):
    from offmark import _hip
    for name in SYMS:
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    assert lib.ofmk_version() == 6


@pytest.mark.parametrize("name", SYMS)
def test_bad_arguments_return_e_arg_without_a_gpu(lib, name):
    writes = name != "ofmk_svd_detect_yuv420"
    assert call(lib, name, inp=None) == E_ARG
    if writes:
        assert call(lib, name, out=None) == E_ARG
    assert call(lib, name, sc=C.cast(None, C.POINTER(C.c_double))) == E_ARG
    assert call(lib, name, h=12) == E_ARG and call(lib, name, w=20) == E_ARG and call(lib, name, h=12, w=20) == E_ARG
    assert call(lib, name, n=0) == E_ARG and call(lib, name, h=0) == E_ARG and call(lib, name, w=-8) == E_ARG
    assert call(lib, name, layout=2) == E_ARG and call(lib, name, layout=-1) == E_ARG
    assert call(lib, name, blk=5) == E_ARG and call(lib, name, blk=2) == E_ARG
    assert call(lib, name, sc=scales(0, float("nan"), 0)) == E_ARG
    assert call(lib, name, sc=scales(float("inf"), 15, 0)) == E_ARG
    if writes:
        assert call(lib, name, sc=scales(0, 0, 0)) == E_ARG and call(lib, name, sc=scales(-1, -15, 0)) == E_ARG
    if name != "ofmk_svd_embed_yuv420":
        assert call(lib, name, l=0) == E_ARG
        assert call(lib, name, counts=None, bits=None) == E_ARG
    assert call(lib, name, inp=IN + 4) == E_ARG
    if writes:
        assert call(lib, name, out=OUT + 1) == E_ARG
    assert "" != lib.ofmk_last_error().decode()


@pytest.mark.parametrize("name", SYMS[1:])
def test_partial_counts_rules(lib, name):
    from offmark import _hip
    o = _hip.Opts(_hip.F_PARTIAL_COUNTS, 0, None)
    assert call(lib, name, counts=None, opts=C.byref(o)) == E_ARG                  # partial form needs a counts buffer
    assert call(lib, name, l=4096, opts=C.byref(o)) == E_ARG                       # ... and L <= 2048
    bad = _hip.Opts(1 << 20, 0, None)
    assert call(lib, name, opts=C.byref(bad)) == E_ARG                             # unknown flag bits
