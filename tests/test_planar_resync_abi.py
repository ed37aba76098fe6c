"""CPU-only: the planar resync entry points (ofmk_svd_sync_scores_yuv420, ofmk_svd_detect_soft_window_yuv420,
ofmk_sync_workspace_bytes_yuv420, ofmk_sync_scores_yuv420, ofmk_detect_soft_window_yuv420; build extensions) are exported, declared
and bound, and refuse bad arguments with OFMK_E_ARG / OFMK_E_WORKSPACE before any HIP call, so these run without a GPU (the pointer
values below are never dereferenced)."""
import ctypes as C
import inspect
import os
import re

import pytest

from conftest import ROOT

E_ARG, E_WORKSPACE = -1, -2
H, W, N, L = 62, 84, 3, 8
IN, OUT, WS = 0x10001, 0x20000, 0x30000          # IN is odd: no alignment is asked of the planes; WS: 256-byte aligned
BIG = 1 << 40                                    # a workspace size that is never too small
SYMS = ("ofmk_svd_sync_scores_yuv420", "ofmk_svd_detect_soft_window_yuv420", "ofmk_sync_workspace_bytes_yuv420",
        "ofmk_sync_scores_yuv420", "ofmk_detect_soft_window_yuv420")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from offmark import _hip
    return _hip.load()


def refused(lib, rc, code=E_ARG):
    return rc == code and lib.ofmk_last_error().decode() != ""


def scales3(v):
    return None if v is None else (C.c_double * 3)(*v)


def svd_scores(lib, inp=IN, layout=0, n=N, h=H, w=W, scales=(0, 15, 0), blk=4, out=OUT, opts=None, code=E_ARG):
    return refused(lib, lib.ofmk_svd_sync_scores_yuv420(inp, layout, n, h, w, scales3(scales), blk, out, None, opts), code)


def svd_window(lib, inp=IN, layout=0, n=N, h=H, w=W, py=6, px=4, canvas_cols=13, base=0, l=L, scales=(0, 15, 0), blk=4, out=OUT, opts=None,
               code=E_ARG):
    return refused(lib, lib.ofmk_svd_detect_soft_window_yuv420(inp, layout, n, h, w, py, px, canvas_cols, base, l, scales3(scales), blk, out,
                                                               None, opts), code)


def dct_scores(lib, inp=IN, layout=0, n=N, h=H, w=W, alpha=20.0, out=OUT, cf=0, ws=WS, nbytes=BIG, opts=None, code=E_ARG):
    return refused(lib, lib.ofmk_sync_scores_yuv420(inp, layout, n, h, w, alpha, out, cf, ws, nbytes, None, opts), code)


def dct_window(lib, inp=IN, layout=0, n=N, h=H, w=W, py=6, px=4, canvas_cols=13, base=0, l=L, alpha=20.0, out=OUT, cf=0, ws=WS, nbytes=BIG,
               opts=None, code=E_ARG):
    return refused(lib, lib.ofmk_detect_soft_window_yuv420(inp, layout, n, h, w, py, px, canvas_cols, base, l, alpha, out, cf, ws, nbytes,
                                                           None, opts), code)


ALL = [svd_scores, svd_window, dct_scores, dct_window]


def test_symbols_are_exported_declared_and_bound(lib):
    from offmark import _hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "offmark_hip.h")).read(), flags=re.S)
    for name in SYMS:
        assert hasattr(lib, name) and name in _hip.SIGNATURES and name in _hip.SYMBOLS
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", header), name
    assert lib.ofmk_version() == 6 == _hip.ABI_VERSION
    assert "OFMK_ABI_VERSION 6" in header


@pytest.mark.parametrize("call", ALL)
def test_shared_argument_checks(lib, call):
    assert call(lib, inp=None) and call(lib, out=None)
    assert call(lib, n=0) and call(lib, n=-2)
    assert call(lib, h=61) and call(lib, w=83) and call(lib, h=9) and call(lib, w=9)          # odd H, odd W
    assert call(lib, h=6) and call(lib, w=6) and call(lib, h=0) and call(lib, w=-8)           # H or W < 8
    assert call(lib, h=1 << 14, w=1 << 14)                                                     # H * W = 2^28
    assert call(lib, layout=2) and call(lib, layout=-1)
    from offmark import _hip
    assert call(lib, opts=C.byref(_hip.Opts(1 << 20, 0, None)))                                # unknown flag bits
    assert call(lib, opts=C.byref(_hip.Opts(0, 65, None)))


@pytest.mark.parametrize("call", [svd_scores, svd_window])
def test_svd_argument_checks(lib, call):
    assert call(lib, blk=8) and call(lib, blk=0)
    assert call(lib, scales=None) and call(lib, scales=(0, float("nan"), 0)) and call(lib, scales=(0, float("inf"), 0))
    assert call(lib, scales=(0, 1e-4, 0))
    assert svd_scores(lib, scales=(10, 0, 20))                                                 # the search reads channel 1


@pytest.mark.parametrize("call", [dct_scores, dct_window])
def test_dct_argument_checks(lib, call):
    assert call(lib, ws=None) and call(lib, ws=WS + 8)
    assert call(lib, alpha=float("nan")) and call(lib, alpha=float("inf")) and call(lib, alpha=0.0) and call(lib, alpha=-20.0)


@pytest.mark.parametrize("call", [svd_window, dct_window])
def test_window_argument_checks(lib, call):
    assert call(lib, py=5) and call(lib, px=3) and call(lib, py=1, px=1)                       # odd phases do not exist on planes
    assert call(lib, py=8) and call(lib, px=8) and call(lib, py=-2) and call(lib, px=-2)
    assert call(lib, h=12, py=6) and call(lib, w=10, px=4)                                     # no full unit at that phase
    assert call(lib, canvas_cols=9) and call(lib, canvas_cols=0)                               # the window has (84 - 4) // 8 = 10 units per row
    assert call(lib, base=-1)
    assert call(lib, base=(1 << 31) - 7 * 13) and call(lib, canvas_cols=1 << 29)               # base + rows * canvas_cols >= 2^31
    assert call(lib, l=0) and call(lib, l=-3)


def test_a_small_workspace_is_refused(lib):
    need = lib.ofmk_sync_workspace_bytes_yuv420(1, H, W)
    assert dct_scores(lib, nbytes=need - 1, code=E_WORKSPACE) and dct_scores(lib, nbytes=0, code=E_WORKSPACE)
    rows, cols = (H - 6) // 8, (W - 4) // 8
    need = lib.ofmk_workspace_bytes(1, 8 * rows, 8 * cols)                                     # the WINDOW's blocks
    assert dct_window(lib, nbytes=need - 1, code=E_WORKSPACE) and dct_window(lib, nbytes=0, code=E_WORKSPACE)


def test_sync_workspace_bytes_yuv420(lib):
    q, rgb = lib.ofmk_sync_workspace_bytes_yuv420, lib.ofmk_sync_workspace_bytes
    assert q(0, H, W) == 0 and q(-1, H, W) == 0 and q(1, 6, W) == 0 and q(1, H, 6) == 0 and q(1, 1 << 14, 1 << 14) == 0
    assert q(1, 61, W) == 0 and q(1, H, 83) == 0                                               # odd sizes
    sizes = [q(k, H, W) for k in (1, 2, 3, 8, 100)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))                                        # monotone in frames
    assert sizes[0] >= (H // 2 - 3) * (W // 2 - 3) * 12 + 16 * 8                               # one record per even origin, 16 sums
    for h, w in ((8, 8), (8, 10), (10, 14), (H, W), (100, 138), (1072, 1904), (1080, 1920)):
        for k in (1, 8):
            assert 0 < q(k, h, w) <= rgb(k, h, w), (h, w, k)
    assert q(8, 1080, 1920) < 0.27 * rgb(8, 1080, 1920)                                        # a quarter of the RGB search's records


def test_engine_and_decoder_methods():
    from offmark import resync
    from offmark.engine import DctEngine
    from offmark.extract.dct_decoder import DctDecoder
    from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder
    for name in ("sync_scores_planes_yuv420", "decode_soft_window_planes_yuv420"):
        assert inspect.signature(getattr(DctDecoder, name)) == inspect.signature(getattr(DwtDctSvdDecoder, name)), name
    assert list(inspect.signature(DctDecoder.sync_scores_planes_yuv420).parameters) == ["self", "planes", "height", "width", "layout"]
    assert list(inspect.signature(DctDecoder.decode_soft_window_planes_yuv420).parameters) == [
        "self", "planes", "height", "width", "L", "phase", "canvas_cols", "base", "layout"]
    par = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert par(DctEngine.svd_sync_scores_yuv420) == ["self", "planes", "H", "W", "scale", "scales", "blk", "layout", "scores"]
    assert par(DctEngine.svd_detect_soft_window_yuv420)[:7] == ["self", "planes", "H", "W", "L", "phase", "canvas_cols"]
    assert par(DctEngine.sync_workspace_yuv420) == ["self", "H", "W", "frames"]
    assert par(DctEngine.sync_scores_yuv420) == ["self", "planes", "H", "W", "alpha", "layout", "scores"]
    assert par(DctEngine.detect_soft_window_yuv420) == ["self", "planes", "H", "W", "L", "phase", "canvas_cols", "base", "alpha", "layout", "soft"]
    assert par(resync.best_phase) == ["scores", "H", "W", "even_only"] and inspect.signature(resync.best_phase).parameters["even_only"].default is False
    assert par(resync.read_cropped_leak_yuv420) == ["decoder", "planes", "height", "width", "segment_of_frame", "canvas_width", "candidates",
                                                    "key", "L", "search_frames", "layout"]
