"""CPU-only: the DCT codec's resync entry points (ofmk_sync_workspace_bytes, ofmk_sync_scores_rgb8, ofmk_detect_soft_window_rgb8;
build extensions) are exported, declared and bound, and refuse bad arguments with OFMK_E_ARG / OFMK_E_WORKSPACE before any HIP
call, so these run without a GPU (the pointer values below are never dereferenced)."""
import ctypes as C
import inspect
import os
import re

import pytest

from conftest import ROOT

E_ARG, E_WORKSPACE = -1, -2
H, W, N, L = 61, 83, 3, 8
IN, OUT, WS = 0x10000, 0x20000, 0x30000          # WS: 256-byte aligned, as the library asks
BIG = 1 << 40                                    # a workspace size that is never too small
SYMS = ("ofmk_sync_workspace_bytes", "ofmk_sync_scores_rgb8", "ofmk_detect_soft_window_rgb8")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from offmark import _hip
    return _hip.load()


def refused(lib, rc, code=E_ARG):
    return rc == code and lib.ofmk_last_error().decode() != ""


def scores(lib, inp=IN, n=N, h=H, w=W, alpha=20.0, out=OUT, cf=0, ws=WS, nbytes=BIG, opts=None, code=E_ARG):
    return refused(lib, lib.ofmk_sync_scores_rgb8(inp, n, h, w, alpha, out, cf, ws, nbytes, None, opts), code)


def window(lib, inp=IN, n=N, h=H, w=W, py=5, px=3, canvas_cols=13, base=0, l=L, alpha=20.0, out=OUT, cf=0, ws=WS, nbytes=BIG, opts=None,
           code=E_ARG):
    return refused(lib, lib.ofmk_detect_soft_window_rgb8(inp, n, h, w, py, px, canvas_cols, base, l, alpha, out, cf, ws, nbytes, None, opts),
                   code)


def test_symbols_are_exported_declared_and_bound(lib):
    from offmark import _hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "offmark_hip.h")).read(), flags=re.S)
    for name in SYMS:
        assert hasattr(lib, name) and name in _hip.SIGNATURES and name in _hip.SYMBOLS
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", header), name
    assert lib.ofmk_version() == 6 == _hip.ABI_VERSION
    assert (E_ARG, E_WORKSPACE) == tuple(int(re.search(r"#define\s+" + k + r"\s+(-?\d+)", header).group(1))
                                         for k in ("OFMK_E_ARG", "OFMK_E_WORKSPACE"))


@pytest.mark.parametrize("call", [scores, window])
def test_shared_argument_checks(lib, call):
    assert call(lib, inp=None) and call(lib, out=None) and call(lib, ws=None)
    assert call(lib, n=0) and call(lib, n=-2)
    assert call(lib, h=7) and call(lib, w=7) and call(lib, h=0) and call(lib, w=-8)
    assert call(lib, h=1 << 14, w=1 << 14)                                          # H * W = 2^28: the SVD call's size bound
    assert call(lib, alpha=float("nan")) and call(lib, alpha=float("inf")) and call(lib, alpha=float("-inf"))
    assert call(lib, alpha=0.0) and call(lib, alpha=-20.0)
    from offmark import _hip
    assert call(lib, opts=C.byref(_hip.Opts(1 << 20, 0, None)))                     # unknown flag bits
    assert call(lib, opts=C.byref(_hip.Opts(0, 65, None)))


def test_a_small_workspace_is_refused(lib):
    need = lib.ofmk_sync_workspace_bytes(1, H, W)
    assert scores(lib, nbytes=need - 1, code=E_WORKSPACE) and scores(lib, nbytes=0, code=E_WORKSPACE)
    rows, cols = (H - 5) // 8, (W - 3) // 8
    need = lib.ofmk_workspace_bytes(1, 8 * rows, 8 * cols)                          # the WINDOW's blocks
    assert window(lib, nbytes=need - 1, code=E_WORKSPACE) and window(lib, nbytes=0, code=E_WORKSPACE)


def test_sync_workspace_bytes(lib):
    q = lib.ofmk_sync_workspace_bytes
    assert q(0, H, W) == 0 and q(-1, H, W) == 0 and q(1, 7, W) == 0 and q(1, H, 7) == 0 and q(1, 1 << 14, 1 << 14) == 0
    sizes = [q(k, H, W) for k in (1, 2, 3, 8, 100)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))                             # monotone in frames
    assert sizes[0] >= (H - 7) * (W - 7) * 12 + 64 * 8                              # one record per pixel origin, 64 sums
    assert q(1, 8, 8) > 0 and q(1, 1080, 1920) >= 1073 * 1913 * 12


def test_window_argument_checks(lib):
    assert window(lib, py=-1) and window(lib, py=8) and window(lib, px=-1) and window(lib, px=8)
    assert window(lib, h=12, py=5) and window(lib, w=10, px=3)                      # no full unit at that phase
    assert window(lib, canvas_cols=9) and window(lib, canvas_cols=0)                # the window has (83 - 3) // 8 = 10 units per row
    assert window(lib, base=-1)
    assert window(lib, base=(1 << 31) - 7 * 13) and window(lib, canvas_cols=1 << 29)     # base + rows * canvas_cols >= 2^31
    assert window(lib, l=0) and window(lib, l=-3)


def test_decoder_and_engine_methods_mirror_the_svd_pair():
    from offmark.engine import DctEngine
    from offmark.extract.dct_decoder import DctDecoder
    from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder
    for name in ("sync_scores_u8", "decode_soft_window_u8"):
        assert inspect.signature(getattr(DctDecoder, name)) == inspect.signature(getattr(DwtDctSvdDecoder, name)), name
    assert list(inspect.signature(DctEngine.sync_scores).parameters) == ["self", "frames", "alpha", "scores"]
    assert list(inspect.signature(DctEngine.detect_soft_window).parameters) == ["self", "frames", "L", "phase", "canvas_cols", "base",
                                                                                 "alpha", "soft"]
    assert list(inspect.signature(DctEngine.sync_workspace).parameters) == ["self", "H", "W", "frames"]
    assert inspect.signature(DctEngine.sync_scores).parameters["alpha"].default == 20
    assert inspect.signature(DctEngine.detect_soft_window).parameters["base"].default == 0
