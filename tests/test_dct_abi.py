"""CPU-only: the DCT codec's single-copy entry points (RGB8, float32 YUV, 4:2:0 planes) are exported and bound, and they refuse
bad arguments before any HIP call -- so these run without a GPU (the pointer values below are never dereferenced).
ofmk_detect_soft_yuv420 has its own in tests/test_svd_soft_abi.py."""
import ctypes as C

import pytest

E_ARG, E_WORKSPACE = -1, -2
H, W, N, L = 64, 96, 3, 8
IN, OUT, WM, ROWS, CNT, BITS, SOFT, WS = 0x1000000, 0x4000000, 0x8000000, 0x9000000, 0xA000000, 0xB000000, 0xD000000, 0xC000000
DEFAULTS = dict(inp=IN, out=OUT, layout=0, n=N, h=H, w=W, wm=WM, n_wm=4, rows=ROWS, l=L, counts=CNT, bits=BITS, soft=SOFT, ws=WS,
                ws_bytes=None, opts=None)
# the arguments of each call between its frames and (chunk_frames, workspace, workspace_bytes, stream, opts), by name in DEFAULTS
# (alpha stands for 20.0); what a call takes decides which refusals apply to it
EMBED = ("n", "h", "w", "wm", "n_wm", "rows", "alpha")
DETECT = ("n", "h", "w", "l", "alpha", "counts", "bits")
CALLS = {
    "ofmk_embed_rgb8": ("inp", "out") + EMBED,
    "ofmk_detect_rgb8": ("inp",) + DETECT,
    "ofmk_detect_soft_rgb8": ("inp", "n", "h", "w", "l", "alpha", "soft"),
    "ofmk_embed_detect_rgb8": ("inp", "out") + EMBED + ("l", "counts", "bits"),
    "ofmk_encode_yuv32f": ("inp",) + EMBED,
    "ofmk_decode_yuv32f": ("inp",) + DETECT,
    "ofmk_embed_yuv420": ("inp", "out", "layout") + EMBED,
    "ofmk_detect_yuv420": ("inp", "layout") + DETECT,
    "ofmk_embed_detect_yuv420": ("inp", "out", "layout") + EMBED + ("l", "counts", "bits"),
}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from offmark import _hip
    return _hip.load()


def call(lib, name, **kw):
    a = dict(DEFAULTS, alpha=20.0, **kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = lib.ofmk_workspace_bytes(max(a["n"], 1), max(a["h"], 8), max(a["w"], 8))
    return getattr(lib, name)(*[a[k] for k in CALLS[name]], 0, a["ws"], a["ws_bytes"], None, a["opts"])


def test_symbols_are_exported_and_bound(lib):
    from offmark import _hip
    for name in CALLS:
        assert hasattr(lib, name) and name in _hip.SIGNATURES and name in _hip.SYMBOLS
    assert lib.ofmk_version() == 6


@pytest.mark.parametrize("name", sorted(CALLS))
def test_bad_arguments_return_e_arg_without_a_gpu(lib, name):
    from offmark import _hip
    takes = CALLS[name]

    def refused(**kw):
        assert all(k in takes or k == "opts" for k in kw), kw           # a case that the call has no argument for proves nothing
        rc = call(lib, name, **kw)
        text = lib.ofmk_last_error().decode()
        return rc == E_ARG and text != ""

    assert refused(inp=None)
    assert refused(n=0) and refused(n=-3)
    assert refused(h=7) and refused(w=7) and refused(h=0, w=0) and refused(h=4, w=4)
    if "out" in takes:
        assert refused(out=None)
    if "wm" in takes:
        assert refused(wm=None)
        assert refused(n_wm=0) and refused(n_wm=-1)
        assert call(lib, name, rows=None, ws_bytes=0) == E_WORKSPACE    # the row map is optional
    if "l" in takes:
        assert refused(l=0) and refused(l=-1)
    if "counts" in takes:
        assert refused(counts=None, bits=None)                          # nothing to read out into
        # either alone is enough: the call gets past the argument checks (to the check of a workspace that is too small)
        assert call(lib, name, counts=None, ws_bytes=0) == E_WORKSPACE and call(lib, name, bits=None, ws_bytes=0) == E_WORKSPACE
        assert refused(l=0, bits=None) and refused(l=-1, counts=None)
    if "soft" in takes:
        assert refused(soft=None)
    if "layout" in takes:
        assert refused(layout=2) and refused(layout=-1)
        assert refused(h=60) and refused(w=44) and refused(h=12, w=12)  # H, W multiples of 8
        assert refused(inp=IN + 1) and refused(inp=IN + 4)              # 8-byte aligned buffers
        if "out" in takes:
            assert refused(out=OUT + 1) and refused(out=OUT + 4)
    else:
        # interleaved frames: any size from 8 up, at any address (the workspace's size is what stops these)
        assert call(lib, name, h=36, w=52, ws_bytes=0) == E_WORKSPACE and call(lib, name, inp=IN + 1, ws_bytes=0) == E_WORKSPACE
    bad = _hip.Opts(1 << 20, 0, None)
    assert refused(opts=C.byref(bad))                                   # unknown flag bits
    both = _hip.Opts(_hip.F_LINEAR_TILES | _hip.F_XCD_TILES, 0, None)
    assert refused(opts=C.byref(both))
    one = _hip.Opts(_hip.F_LINEAR_TILES, 0, None)
    assert call(lib, name, opts=C.byref(one), ws_bytes=0) == E_WORKSPACE


@pytest.mark.parametrize("name", sorted(CALLS))
def test_workspace_is_checked_after_the_arguments(lib, name):
    need = lib.ofmk_workspace_bytes(1, H, W)
    assert need > 0
    # an otherwise valid call gets as far as the workspace's size: every check in front of it passed
    assert call(lib, name, ws_bytes=0) == E_WORKSPACE
    assert "workspace" in lib.ofmk_last_error().decode()
    assert call(lib, name, ws_bytes=need - 1) == E_WORKSPACE
    assert call(lib, name, n=1, ws_bytes=need - 1) == E_WORKSPACE
    # a null or misaligned workspace is a bad argument, whatever its size
    for ws in (None, WS + 8, WS + 128):
        assert call(lib, name, ws=ws) == E_ARG
        assert "workspace" in lib.ofmk_last_error().decode()
    # and a bad argument is reported ahead of a bad workspace
    assert call(lib, name, n=0, ws_bytes=0) == E_ARG and call(lib, name, inp=None, ws=None) == E_ARG
