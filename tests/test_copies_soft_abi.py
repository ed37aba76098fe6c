"""CPU-only: the copies calls with the soft read-out (ofmk_embed_detect_copies_soft_rgb8, ofmk_svd_embed_copies_soft_rgb8,
ofmk_svd_embed_copies_soft_yuv420) are exported and bound, and they refuse bad arguments before any HIP call -- so these run
without a GPU (the pointer values below are never dereferenced)."""
import ctypes as C

import pytest

E_ARG, E_WORKSPACE = -1, -2
H, W, N, L, COPIES = 64, 96, 3, 8, 3
IN, OUT, WM, ROWS, CNT, BITS, SOFT, WS = 0x1000000, 0x4000000, 0x8000000, 0x9000000, 0xA000000, 0xB000000, 0xD000000, 0xC000000
SYMS = ("ofmk_embed_detect_copies_soft_rgb8", "ofmk_svd_embed_copies_soft_rgb8", "ofmk_svd_embed_copies_soft_yuv420")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from offmark import _hip
    return _hip.load()


def dct(lib, inp=IN, out=OUT, copies=COPIES, n=N, h=H, w=W, wm=WM, n_wm=4, rows=ROWS, l=L, counts=CNT, bits=BITS, soft=SOFT,
        ws_bytes=None, opts=None):
    if ws_bytes is None:
        ws_bytes = lib.ofmk_copies_workspace_bytes(n if n > 0 else 1, min(max(copies, 1), 16), max(h, 8), max(w, 8))
    return lib.ofmk_embed_detect_copies_soft_rgb8(inp, out, copies, n, h, w, wm, n_wm, rows, 20.0, l, counts, bits, soft, 0, WS,
                                                  ws_bytes, None, opts)


def svd(lib, inp=IN, out=OUT, copies=COPIES, n=N, h=H, w=W, wm=WM, n_wm=4, rows=ROWS, l=L, counts=CNT, bits=BITS, soft=SOFT,
        blk=4, opts=None):
    from offmark import _hip
    return lib.ofmk_svd_embed_copies_soft_rgb8(inp, out, copies, n, h, w, wm, n_wm, rows, _hip.scales3(15), blk, l, counts, bits, soft,
                                               None, opts)


def planar(lib, inp=IN, out=OUT, layout=0, copies=COPIES, n=N, h=H, w=W, wm=WM, n_wm=4, rows=ROWS, l=L, counts=CNT, bits=BITS,
           soft=SOFT, blk=4, opts=None):
    from offmark import _hip
    return lib.ofmk_svd_embed_copies_soft_yuv420(inp, out, layout, copies, n, h, w, wm, n_wm, rows, _hip.scales3(15), blk, l, counts,
                                                 bits, soft, None, opts)


CALLS = {"dct": (dct, H * W * 3), "svd": (svd, H * W * 3), "planar": (planar, H * W * 3 // 2)}


def test_symbols_are_exported_and_bound(lib):
    from offmark import _hip
    for name in SYMS:
        assert hasattr(lib, name) and name in _hip.SIGNATURES and name in _hip.SYMBOLS
    assert lib.ofmk_version() == 6


@pytest.mark.parametrize("which", sorted(CALLS))
def test_bad_arguments_return_e_arg_without_a_gpu(lib, which):
    from offmark import _hip
    call, frame_bytes = CALLS[which]
    batch = N * frame_bytes

    def refused(**kw):
        rc = call(lib, **kw)
        text = lib.ofmk_last_error().decode()
        return rc == E_ARG and text != ""

    assert refused(soft=None)
    assert refused(soft=None, counts=None, bits=None)
    assert refused(inp=None) and refused(out=None) and refused(wm=None)
    assert refused(copies=0) and refused(copies=17) and refused(copies=-1)
    assert refused(n=0) and refused(n=-3)
    assert refused(l=0) and refused(l=-1) and refused(l=0, counts=None, bits=None)
    assert refused(h=7) and refused(w=4) and refused(h=0, w=0)
    assert refused(n_wm=0)
    assert refused(out=IN)                                              # in place
    assert refused(out=IN + batch // 2 // 8 * 8)                        # out starts inside in
    assert refused(inp=OUT + 2 * batch + 8)                             # in starts inside the third copy of out
    assert refused(inp=OUT + COPIES * batch - 8)                        # ... inside the end of out
    bad = _hip.Opts(1 << 20, 0, None)
    assert refused(opts=C.byref(bad))                                   # unknown flag bits
    if which != "dct":
        assert refused(blk=5) and refused(blk=0)
        big = _hip.Opts(_hip.F_PARTIAL_COUNTS, 0, None)
        assert refused(opts=C.byref(big), counts=None)                  # partial counts without a counts buffer
        assert refused(opts=C.byref(big), l=4096)                       # ... and past the LDS histogram
    if which == "planar":
        assert refused(layout=2) and refused(layout=-1)
        assert refused(h=60) and refused(w=100)                         # H, W multiples of 8
        assert refused(inp=IN + 4) and refused(out=OUT + 2)             # 8-byte aligned buffers


def test_dct_call_takes_the_copies_workspace(lib):
    need = lib.ofmk_copies_workspace_bytes(1, COPIES, H, W)
    assert need > 0
    assert dct(lib, ws_bytes=need - 1) == E_WORKSPACE
    assert "workspace" in lib.ofmk_last_error().decode()
    assert dct(lib, ws_bytes=lib.ofmk_workspace_bytes(1, H, W)) == E_WORKSPACE
