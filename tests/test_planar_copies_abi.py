"""CPU-only: the planar copies entry points (ofmk_embed_copies_yuv420, ofmk_svd_embed_copies_yuv420) are exported and refuse bad
arguments before any HIP call, so these run without a GPU.  The pointer values below are fake addresses that are never
dereferenced: every call in this file is one the library refuses."""
import ctypes as C

import pytest

E_ARG, E_WORKSPACE = -1, -2
H, W, N, L, COPIES = 64, 96, 3, 8, 3
FRAME_BYTES = N * H * W * 3 // 2                      # one copy: n frames of 1.5*H*W bytes
IN, OUT, WM, ROWS, CNT, BITS, WS = 0x1000000, 0x4000000, 0x8000000, 0x9000000, 0xA000000, 0xB000000, 0xC000000
I420, NV12 = 0, 1
SYMS = ("ofmk_embed_copies_yuv420", "ofmk_svd_embed_copies_yuv420")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from offmark import _hip
    return _hip.load()


def scales(*v):
    return (C.c_double * 3)(*v)


def dct(lib, inp=IN, out=OUT, layout=I420, copies=COPIES, n=N, h=H, w=W, wm=WM, n_wm=4, rows=ROWS, ws_bytes=None, opts=None):
    if ws_bytes is None:
        ws_bytes = lib.ofmk_workspace_bytes(n if n > 0 else 1, max(h, 8), max(w, 8))
    return lib.ofmk_embed_copies_yuv420(inp, out, layout, copies, n, h, w, wm, n_wm, rows, 20.0, 0, WS, ws_bytes, None, opts)


def svd(lib, inp=IN, out=OUT, layout=I420, copies=COPIES, n=N, h=H, w=W, wm=WM, n_wm=4, rows=ROWS, sc=None, blk=4, l=L,
        counts=CNT, bits=BITS, opts=None):
    sc = scales(0, 15, 0) if sc is None else sc
    return lib.ofmk_svd_embed_copies_yuv420(inp, out, layout, copies, n, h, w, wm, n_wm, rows, sc, blk, l, counts, bits, None, opts)


CALLS = {"ofmk_embed_copies_yuv420": dct, "ofmk_svd_embed_copies_yuv420": svd}


def test_symbols_are_exported_and_bound(lib):
    from offmark import _hip
    for name in SYMS:
        assert hasattr(lib, name) and name in _hip.SIGNATURES and name in _hip.SYMBOLS
    assert lib.ofmk_version() == 6


@pytest.mark.parametrize("layout", [I420, NV12])
@pytest.mark.parametrize("name", SYMS)
def test_bad_arguments_return_e_arg_without_a_gpu(lib, name, layout):
    from offmark import _hip
    call = CALLS[name]

    def refused(**kw):
        kw.setdefault("layout", layout)
        rc = call(lib, **kw)
        text = lib.ofmk_last_error().decode()
        return rc == E_ARG and text != ""

    assert refused(inp=None) and refused(out=None) and refused(wm=None)
    assert refused(copies=0) and refused(copies=17) and refused(copies=-1)
    assert refused(n=0) and refused(n=-3)
    assert refused(h=7) and refused(w=4) and refused(h=0, w=0)          # below 8
    assert refused(h=H + 4) and refused(w=W + 4) and refused(h=H + 1)   # not a multiple of 8
    assert refused(layout=2) and refused(layout=-1)
    assert refused(inp=IN + 4) and refused(out=OUT + 2)                 # not 8-byte aligned
    assert refused(n_wm=0)
    assert refused(out=IN)                                              # in place
    assert refused(out=IN + FRAME_BYTES // 2)                           # out starts inside in
    assert refused(inp=OUT + 2 * FRAME_BYTES + 8)                       # in starts inside the third copy of out
    # ... inside the last 8 bytes of out, counted with 1.5*H*W bytes per frame (a copy of H*W*3 bytes would end far beyond)
    assert refused(inp=OUT + COPIES * FRAME_BYTES - 8)
    assert refused(out=IN - COPIES * FRAME_BYTES + 8)                   # the last copy of out runs into in
    bad = _hip.Opts(1 << 20, 0, None)
    assert refused(opts=C.byref(bad))                                   # unknown flag bits


def test_svd_specific_arguments(lib):
    from offmark import _hip

    def refused(**kw):
        return svd(lib, **kw) == E_ARG and lib.ofmk_last_error().decode() != ""

    assert refused(sc=C.cast(None, C.POINTER(C.c_double)))
    assert refused(sc=scales(0, float("nan"), 0)) and refused(sc=scales(float("inf"), 15, 0))
    assert refused(sc=scales(0, 0, 0)) and refused(sc=scales(-1, -15, 0))
    assert refused(blk=5) and refused(blk=2) and refused(blk=16) and refused(blk=0)
    assert refused(l=0) and refused(l=0, bits=None) and refused(l=-1, counts=None)
    o = _hip.Opts(_hip.F_PARTIAL_COUNTS, 0, None)
    assert refused(counts=None, opts=C.byref(o))                        # partial form needs a counts buffer
    assert refused(l=4096, opts=C.byref(o))                             # ... and L <= 2048
    assert refused(blk=8, l=4096, opts=C.byref(o))


def test_dct_workspace_too_small(lib):
    need = lib.ofmk_workspace_bytes(1, H, W)
    assert need > 0
    for layout in (I420, NV12):
        assert dct(lib, layout=layout, ws_bytes=need - 1) == E_WORKSPACE
        assert dct(lib, layout=layout, ws_bytes=0) == E_WORKSPACE
        assert "workspace" in lib.ofmk_last_error().decode()
