"""CPU-only: the DCT codec's copies-with-verify entry points (ofmk_embed_detect_copies_rgb8, ofmk_copies_workspace_bytes) are
exported and bound, the call refuses bad arguments before any HIP call, and the sizing function is monotone -- so these run
without a GPU (the pointer values below are never dereferenced)."""
import ctypes as C

import pytest

E_ARG, E_WORKSPACE = -1, -2
H, W, N, L, COPIES = 64, 96, 3, 8, 3
FRAME_BYTES = N * H * W * 3
IN, OUT, WM, ROWS, CNT, BITS, WS = 0x1000000, 0x4000000, 0x8000000, 0x9000000, 0xA000000, 0xB000000, 0xC000000
SYMS = ("ofmk_embed_detect_copies_rgb8", "ofmk_copies_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from offmark import _hip
    return _hip.load()


def call(lib, inp=IN, out=OUT, copies=COPIES, n=N, h=H, w=W, wm=WM, n_wm=4, rows=ROWS, l=L, counts=CNT, bits=BITS, ws_bytes=None,
         opts=None):
    if ws_bytes is None:
        ws_bytes = lib.ofmk_copies_workspace_bytes(n if n > 0 else 1, min(max(copies, 1), 16), max(h, 8), max(w, 8))
    return lib.ofmk_embed_detect_copies_rgb8(inp, out, copies, n, h, w, wm, n_wm, rows, 20.0, l, counts, bits, 0, WS, ws_bytes,
                                             None, opts)


def test_symbols_are_exported_and_bound(lib):
    from offmark import _hip
    for name in SYMS:
        assert hasattr(lib, name) and name in _hip.SIGNATURES and name in _hip.SYMBOLS
    assert lib.ofmk_version() == 6


def test_bad_arguments_return_e_arg_without_a_gpu(lib):
    from offmark import _hip

    def refused(**kw):
        rc = call(lib, **kw)
        text = lib.ofmk_last_error().decode()
        return rc == E_ARG and text != ""

    assert refused(inp=None) and refused(out=None) and refused(wm=None)
    assert refused(counts=None, bits=None)                              # nothing to read out into
    assert refused(copies=0) and refused(copies=17) and refused(copies=-1)
    assert refused(n=0) and refused(n=-3)
    assert refused(h=7) and refused(w=4) and refused(h=0, w=0)
    assert refused(n_wm=0)
    assert refused(l=0) and refused(l=-1) and refused(l=0, bits=None) and refused(l=-1, counts=None)
    assert refused(out=IN)                                              # in place
    assert refused(out=IN + FRAME_BYTES // 2)                           # out starts inside in
    assert refused(inp=OUT + 2 * FRAME_BYTES + 5)                       # in starts inside the third copy of out
    assert refused(inp=OUT + COPIES * FRAME_BYTES - 1)                  # ... inside the last byte of out
    bad = _hip.Opts(1 << 20, 0, None)
    assert refused(opts=C.byref(bad))                                   # unknown flag bits
    both = _hip.Opts(_hip.F_LINEAR_TILES | _hip.F_XCD_TILES, 0, None)
    assert refused(opts=C.byref(both))                                  # both tile orders at once


def test_workspace_too_small(lib):
    need = lib.ofmk_copies_workspace_bytes(1, COPIES, H, W)
    assert need > 0
    assert call(lib, ws_bytes=need - 1) == E_WORKSPACE
    assert "workspace" in lib.ofmk_last_error().decode()
    assert call(lib, ws_bytes=0) == E_WORKSPACE
    # what is enough for the single-copy calls is not enough here: every copy keeps records of its own
    assert call(lib, ws_bytes=lib.ofmk_workspace_bytes(1, H, W)) == E_WORKSPACE


def test_copies_workspace_bytes(lib):
    size = lib.ofmk_copies_workspace_bytes
    assert size(1, 0, H, W) == 0 and size(1, 17, H, W) == 0 and size(1, -1, H, W) == 0
    assert size(1, COPIES, 7, W) == 0 and size(1, COPIES, H, 4) == 0 and size(0, COPIES, H, W) == 0
    for h, w in ((H, W), (16, 24), (250, 330), (1080, 1920)):
        by_frames = [size(f, COPIES, h, w) for f in (1, 2, 3, 7, 300)]
        assert by_frames[0] > 0 and all(a < b for a, b in zip(by_frames, by_frames[1:])), (h, w, by_frames)
        by_copies = [size(2, c, h, w) for c in range(1, 17)]
        assert by_copies[0] > 0 and all(a < b for a, b in zip(by_copies, by_copies[1:])), (h, w, by_copies)
        for f in (1, 2, 300):
            for c in (1, 2, 16):
                assert size(f, c, h, w) >= lib.ofmk_workspace_bytes(f, h, w), (h, w, f, c)
