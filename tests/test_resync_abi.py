"""CPU-only: the resync entry points (ofmk_svd_sync_scores_rgb8, ofmk_svd_detect_soft_window_rgb8; build extensions) are exported,
declared and bound, and refuse bad arguments with OFMK_E_ARG before any HIP call, so these run without a GPU (the pointer
values below are never dereferenced)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

E_ARG = -1
H, W, N, L = 61, 83, 3, 8
IN, OUT = 0x10000, 0x20000
SYMS = ("ofmk_svd_sync_scores_rgb8", "ofmk_svd_detect_soft_window_rgb8")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from offmark import _hip
    return _hip.load()


def scales(*v):
    return (C.c_double * 3)(*v)


def refused(lib, rc):
    return rc == E_ARG and lib.ofmk_last_error().decode() != ""


def scores(lib, inp=IN, n=N, h=H, w=W, sc=None, blk=4, out=OUT, opts=None):
    sc = scales(0, 15, 0) if sc is None else sc
    return refused(lib, lib.ofmk_svd_sync_scores_rgb8(inp, n, h, w, sc, blk, out, None, opts))


def window(lib, inp=IN, n=N, h=H, w=W, py=5, px=3, canvas_cols=13, base=0, l=L, sc=None, blk=4, out=OUT, opts=None):
    sc = scales(0, 15, 0) if sc is None else sc
    return refused(lib, lib.ofmk_svd_detect_soft_window_rgb8(inp, n, h, w, py, px, canvas_cols, base, l, sc, blk, out, None, opts))


def test_symbols_are_exported_declared_and_bound(lib):
    from offmark import _hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "offmark_hip.h")).read(), flags=re.S)
    for name in SYMS:
        assert hasattr(lib, name) and name in _hip.SIGNATURES and name in _hip.SYMBOLS
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert lib.ofmk_version() == 6 == _hip.ABI_VERSION


@pytest.mark.parametrize("call", [scores, window])
def test_shared_argument_checks(lib, call):
    null_scales = C.cast(None, C.POINTER(C.c_double))
    assert call(lib, inp=None) and call(lib, out=None) and call(lib, sc=null_scales)
    assert call(lib, n=0) and call(lib, n=-2)
    assert call(lib, h=7) and call(lib, w=7) and call(lib, h=0) and call(lib, w=-8)
    assert call(lib, h=1 << 14, w=1 << 14)                                          # H * W = 2^28
    assert call(lib, blk=8) and call(lib, blk=5) and call(lib, blk=0)
    assert call(lib, sc=scales(0, float("nan"), 0)) and call(lib, sc=scales(float("inf"), 15, 0)) and call(lib, sc=scales(0, 15, float("-inf")))
    assert call(lib, sc=scales(0, 1e-4, 0)) and call(lib, sc=scales(1e-6, 15, 0))   # a positive scale below 1e-3
    from offmark import _hip
    assert call(lib, opts=C.byref(_hip.Opts(1 << 20, 0, None)))                     # unknown flag bits
    assert call(lib, opts=C.byref(_hip.Opts(0, 65, None)))


def test_scores_need_a_marked_channel_1(lib):
    assert scores(lib, sc=scales(0, 0, 0)) and scores(lib, sc=scales(10, 0, 20)) and scores(lib, sc=scales(0, -15, 0))


def test_window_argument_checks(lib):
    assert window(lib, py=-1) and window(lib, py=8) and window(lib, px=-1) and window(lib, px=8)
    assert window(lib, h=12, py=5) and window(lib, w=10, px=3)                      # no full unit at that phase
    assert window(lib, canvas_cols=9) and window(lib, canvas_cols=0)                # the window has (83 - 3) // 8 = 10 units per row
    assert window(lib, base=-1)
    assert window(lib, base=(1 << 31) - 7 * 13) and window(lib, canvas_cols=1 << 29)     # base + rows * canvas_cols >= 2^31
    assert window(lib, l=0) and window(lib, l=-3)
