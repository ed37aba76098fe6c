"""CPU-only: the DCT codec's copies-with-verify entry points on 4:2:0 planes (ofmk_embed_detect_copies_yuv420,
ofmk_embed_detect_copies_soft_yuv420) are exported and bound, and they refuse bad arguments before any HIP call -- so these run
without a GPU (the pointer values below are never dereferenced)."""
import ctypes as C

import pytest

E_ARG, E_WORKSPACE = -1, -2
H, W, N, L, COPIES = 64, 96, 3, 8, 3
BATCH = N * H * W * 3 // 2                       # bytes of one copy: n frames of 1.5 * H * W
IN, OUT, WM, ROWS, CNT, BITS, SOFT, WS = 0x1000000, 0x4000000, 0x8000000, 0x9000000, 0xA000000, 0xB000000, 0xD000000, 0xC000000
SYMS = ("ofmk_embed_detect_copies_yuv420", "ofmk_embed_detect_copies_soft_yuv420")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from offmark import _hip
    return _hip.load()


def _ws_bytes(lib, copies, n, h, w):
    return lib.ofmk_copies_workspace_bytes(n if n > 0 else 1, min(max(copies, 1), 16), max(h, 8), max(w, 8))


def hard(lib, inp=IN, out=OUT, layout=0, copies=COPIES, n=N, h=H, w=W, wm=WM, n_wm=4, rows=ROWS, l=L, counts=CNT, bits=BITS,
         ws_bytes=None, opts=None):
    if ws_bytes is None:
        ws_bytes = _ws_bytes(lib, copies, n, h, w)
    return lib.ofmk_embed_detect_copies_yuv420(inp, out, layout, copies, n, h, w, wm, n_wm, rows, 20.0, l, counts, bits, 0, WS,
                                               ws_bytes, None, opts)


def soft(lib, inp=IN, out=OUT, layout=0, copies=COPIES, n=N, h=H, w=W, wm=WM, n_wm=4, rows=ROWS, l=L, counts=CNT, bits=BITS,
         soft=SOFT, ws_bytes=None, opts=None):
    if ws_bytes is None:
        ws_bytes = _ws_bytes(lib, copies, n, h, w)
    return lib.ofmk_embed_detect_copies_soft_yuv420(inp, out, layout, copies, n, h, w, wm, n_wm, rows, 20.0, l, counts, bits, soft, 0,
                                                    WS, ws_bytes, None, opts)


CALLS = {"hard": hard, "soft": soft}


def test_symbols_are_exported_and_bound(lib):
    from offmark import _hip
    for name in SYMS:
        assert hasattr(lib, name) and name in _hip.SIGNATURES and name in _hip.SYMBOLS
    assert lib.ofmk_version() == 6


@pytest.mark.parametrize("which", sorted(CALLS))
def test_bad_arguments_return_e_arg_without_a_gpu(lib, which):
    from offmark import _hip
    call = CALLS[which]

    def refused(**kw):
        rc = call(lib, **kw)
        text = lib.ofmk_last_error().decode()
        return rc == E_ARG and text != ""

    assert refused(inp=None) and refused(out=None) and refused(wm=None)
    if which == "hard":
        assert refused(counts=None, bits=None)                          # nothing to read out into
        # either alone is enough: the call gets past the argument checks (to the check of a workspace that is too small)
        assert call(lib, counts=None, ws_bytes=0) == E_WORKSPACE and call(lib, bits=None, ws_bytes=0) == E_WORKSPACE
    else:
        assert refused(soft=None) and refused(soft=None, counts=None, bits=None)
    assert refused(l=0) and refused(l=-1) and refused(l=0, bits=None) and refused(l=-1, counts=None)
    assert refused(copies=0) and refused(copies=17) and refused(copies=-1)
    assert refused(n=0) and refused(n=-3)
    assert refused(n_wm=0)
    assert refused(layout=2) and refused(layout=-1)
    assert refused(h=60) and refused(w=44) and refused(h=0, w=0)        # H, W multiples of 8
    assert refused(inp=IN + 1) and refused(out=OUT + 1) and refused(inp=IN + 4)      # 8-byte aligned buffers
    assert refused(out=IN)                                              # in place
    assert refused(out=IN + BATCH // 2 // 8 * 8)                        # out starts inside in
    assert refused(inp=OUT + (COPIES - 1) * BATCH + 8)                  # in starts inside the last copy of out
    assert refused(inp=OUT + COPIES * BATCH - 8)                        # ... inside the end of out
    assert call(lib, inp=OUT + COPIES * BATCH, ws_bytes=0) == E_WORKSPACE          # right behind out: no overlap
    bad = _hip.Opts(1 << 20, 0, None)
    assert refused(opts=C.byref(bad))                                   # unknown flag bits
    both = _hip.Opts(_hip.F_LINEAR_TILES | _hip.F_XCD_TILES, 0, None)
    assert refused(opts=C.byref(both))


def test_soft_call_without_counts_and_bits_is_not_refused_for_that(lib):
    """The soft sums alone: with a workspace that is too small the call gets past the argument checks to the workspace's."""
    assert soft(lib, counts=None, bits=None, ws_bytes=0) == E_WORKSPACE
    assert hard(lib, counts=None, bits=None, ws_bytes=0) == E_ARG


@pytest.mark.parametrize("which", sorted(CALLS))
def test_workspace_too_small(lib, which):
    call = CALLS[which]
    need = lib.ofmk_copies_workspace_bytes(1, COPIES, H, W)
    assert need > 0
    assert call(lib, ws_bytes=need - 1) == E_WORKSPACE
    assert "workspace" in lib.ofmk_last_error().decode()
    assert call(lib, ws_bytes=0) == E_WORKSPACE
    # what is enough for ofmk_embed_copies_yuv420 is not enough here: every copy keeps records of its own
    assert call(lib, ws_bytes=lib.ofmk_workspace_bytes(1, H, W)) == E_WORKSPACE
