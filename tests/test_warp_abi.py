"""CPU-only: the rescaled-leak entry points (ofmk_warp_units, ofmk_warp_rgb8, ofmk_svd_warp_scores_rgb8,
ofmk_svd_detect_soft_warp_rgb8; build extensions) are exported, declared and bound, and refuse bad arguments with OFMK_E_ARG
before any HIP call, so these run without a GPU (the pointer values below are never dereferenced).  ofmk_warp_units is host
code: it is held against offmark.resync.warp_units and against the per-pixel statement of tests/_warp.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import _warp as wp

E_ARG = -1
h, w, H, W, N, L, K = 61, 83, 72, 104, 3, 8, 5
IN, OUT, CANDS = 0x10000, 0x20000, 0x30000
SYMS = ("ofmk_warp_units", "ofmk_warp_rgb8", "ofmk_svd_warp_scores_rgb8", "ofmk_svd_detect_soft_warp_rgb8")
ONE = 65536


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from offmark import _hip
    return _hip.load()


def scales(*v):
    return (C.c_double * 3)(*v)


def geom(ay=ONE, by=0, ax=ONE, bx=0):
    from offmark import _hip
    return C.byref(_hip.Warp(ay, by, ax, bx))


def refused(lib, rc):
    return rc == E_ARG and lib.ofmk_last_error().decode() != ""


def warp(lib, inp=IN, n=N, lh=h, lw=w, out=OUT, ho=H, wo=W, oy=0, ox=0, g=None, opts=None, **kw):
    g = geom(**kw) if g is None else g
    return refused(lib, lib.ofmk_warp_rgb8(inp, n, lh, lw, out, ho, wo, oy, ox, g, None, opts))


def scores(lib, inp=IN, n=N, lh=h, lw=w, ch=H, cw=W, cands=CANDS, k=K, sc=None, blk=4, out=OUT, opts=None):
    sc = scales(0, 15, 0) if sc is None else sc
    return refused(lib, lib.ofmk_svd_warp_scores_rgb8(inp, n, lh, lw, ch, cw, cands, k, sc, blk, out, None, opts))


def readout(lib, inp=IN, n=N, lh=h, lw=w, ch=H, cw=W, g=None, l=L, sc=None, blk=4, out=OUT, opts=None, **kw):
    sc = scales(0, 15, 0) if sc is None else sc
    g = geom(**kw) if g is None else g
    return refused(lib, lib.ofmk_svd_detect_soft_warp_rgb8(inp, n, lh, lw, ch, cw, g, l, sc, blk, out, None, opts))


def units(lib, lh=h, lw=w, ch=H, cw=W, g=None, out=True, **kw):
    g = geom(**kw) if g is None else g
    r = (C.c_int * 4)(9, 9, 9, 9)
    return lib.ofmk_warp_units(lh, lw, ch, cw, g, r if out else None), tuple(r)


def test_symbols_are_exported_declared_and_bound(lib):
    from offmark import _hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "offmark_hip.h")).read(), flags=re.S)
    for name in SYMS:
        assert hasattr(lib, name) and name in _hip.SIGNATURES and name in _hip.SYMBOLS
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert re.search(r"typedef\s+struct\s+ofmk_warp\s*\{\s*int64_t\s+ay\s*,\s*by\s*,\s*ax\s*,\s*bx\s*;\s*\}\s*ofmk_warp\s*;", header)
    assert C.sizeof(_hip.Warp) == 32
    assert lib.ofmk_version() == 6 == _hip.ABI_VERSION


@pytest.mark.parametrize("call", [warp, scores, readout])
def test_shared_argument_checks(lib, call):
    from offmark import _hip
    assert call(lib, inp=None) and call(lib, out=None)
    assert call(lib, n=0) and call(lib, n=-2)
    assert call(lib, lh=0) and call(lib, lw=0) and call(lib, lh=-8) and call(lib, lh=1 << 14, lw=1 << 14)
    assert call(lib, opts=C.byref(_hip.Opts(1 << 20, 0, None)))                     # unknown flag bits
    assert call(lib, opts=C.byref(_hip.Opts(0, 65, None)))


@pytest.mark.parametrize("call", [warp, readout])
def test_the_map_must_be_in_range(lib, call):
    null_geom = C.cast(None, C.POINTER(__import__("offmark._hip", fromlist=["Warp"]).Warp))
    assert call(lib, g=null_geom)
    assert call(lib, ay=(1 << 12) - 1) and call(lib, ax=(1 << 12) - 1) and call(lib, ay=(1 << 20) + 1) and call(lib, ax=(1 << 20) + 1)
    assert call(lib, ay=0) and call(lib, ax=-ONE)
    assert call(lib, by=(1 << 48) + 1) and call(lib, bx=-(1 << 48) - 1)


def test_warp_argument_checks(lib):
    assert warp(lib, ho=0) and warp(lib, wo=0) and warp(lib, ho=1 << 14, wo=1 << 14)
    assert warp(lib, oy=-1) and warp(lib, ox=-1) and warp(lib, oy=1 << 28)


@pytest.mark.parametrize("call", [scores, readout])
def test_fused_argument_checks(lib, call):
    null_scales = C.cast(None, C.POINTER(C.c_double))
    assert call(lib, sc=null_scales)
    assert call(lib, ch=7) and call(lib, cw=7) and call(lib, ch=1 << 14, cw=1 << 14)   # the canvas holds a unit and H * W < 2^28
    assert call(lib, blk=8) and call(lib, blk=5) and call(lib, blk=0)
    assert call(lib, sc=scales(0, float("nan"), 0)) and call(lib, sc=scales(float("inf"), 15, 0)) and call(lib, sc=scales(0, 1e-4, 0))


def test_scores_argument_checks(lib):
    assert scores(lib, cands=None)
    assert scores(lib, k=0) and scores(lib, k=-1)
    assert scores(lib, sc=scales(0, 0, 0)) and scores(lib, sc=scales(10, 0, 20))       # the search reads channel 1


def test_readout_argument_checks(lib):
    assert readout(lib, l=0) and readout(lib, l=-3)


def test_units_argument_checks(lib):
    null_geom = C.cast(None, C.POINTER(__import__("offmark._hip", fromlist=["Warp"]).Warp))
    assert units(lib, g=null_geom)[0] == E_ARG and units(lib, out=False)[0] == E_ARG
    assert units(lib, lh=0)[0] == E_ARG and units(lib, cw=0)[0] == E_ARG and units(lib, ay=1 << 21)[0] == E_ARG
    assert units(lib, ch=1 << 14, cw=1 << 14)[0] == E_ARG


# leak sizes x canvases x maps: the identity, whole-pixel shifts either way, negative and large offsets, zooms in and out, the
# recipe's geometries, maps that leave no unit, the range's ends
UNIT_LEAKS = [(61, 83), (72, 104), (5, 6), (8, 8), (1, 1), (54, 80)]
UNIT_CANVASES = [(72, 104), (8, 8), (7, 30), (100, 139)]


def unit_maps():
    from offmark import resync
    maps = [wp.IDENTITY, (ONE, 3 << 16, ONE, -(5 << 16)), (ONE, -(11 << 16), ONE, -(21 << 16)), (ONE, -1, ONE, 0), (ONE, 0, ONE, -1),
            (ONE, 1, ONE, 65535), (49152, -20000, 98304, 12345), (98304, 7, 49152, -400000), (32768, 0, 32768, 0), (16384, -70000, 20000, 5),
            (1 << 12, 0, 1 << 12, -(1 << 12)), (1 << 20, 0, 1 << 20, 0), (1 << 20, -(40 << 16), 1 << 18, -(1 << 30)), (ONE, 1 << 40, ONE, 0),
            (ONE, 0, ONE, -(1 << 40)), (ONE + 1, -3, ONE - 1, 3)]
    maps += [resync.warp_of_crop(*wp.CROP, *hw) for hw in (wp.ZOOM_HW, wp.DOWN_HW)]
    maps += [resync.warp_of_crop(0, 0, 72, 104, 108, 156), resync.warp_of_crop(11, 21, 56, 80, 72, 104)]
    return maps


def test_units_equal_the_numpy_helper_and_the_per_pixel_statement(lib):
    from offmark import resync
    seen = set()
    for leak in UNIT_LEAKS:
        for canvas in UNIT_CANVASES:
            for m in unit_maps():
                rc, got = units(lib, lh=leak[0], lw=leak[1], ch=canvas[0], cw=canvas[1], ay=m[0], by=m[1], ax=m[2], bx=m[3])
                assert rc == 0, (leak, canvas, m, lib.ofmk_last_error())
                assert got == resync.warp_units(leak, canvas, m) == wp.units(leak, canvas, m), (leak, canvas, m, got)
                seen.add(got[1] > got[0])
    assert seen == {True, False}
    assert units(lib, lh=72, lw=104)[1] == (0, 9, 0, 13)                       # the identity on the uncropped frame: every unit
    assert units(lib, lh=5, lw=6, ch=8, cw=8)[1] == (0, 0, 0, 0)               # a leak smaller than a unit, not upscaled
    assert units(lib, lh=5, lw=6, ch=16, cw=16, ay=32768, ax=32768)[1] == (0, 1, 0, 1)     # ... upscaled 2x it fills one
    assert units(lib, by=-(11 << 16), bx=-(21 << 16))[1] == (2, 9, 3, 13)      # the cropped recipe: rows 11.., columns 21..


def test_warp_of_crop_and_crop_candidates():
    from offmark import resync
    assert resync.warp_of_crop(0, 0, 72, 104, 72, 104) == wp.IDENTITY
    assert resync.warp_of_crop(11, 21, 61, 83, 61, 83) == (ONE, -(11 << 16), ONE, -(21 << 16))      # a pure crop: a whole-pixel shift
    ay, by, ax, bx = resync.warp_of_crop(*wp.CROP, *wp.ZOOM_HW)
    assert ay == round(72 / 62 * ONE) and ax == round(104 / 92 * ONE)
    assert by == round(((0.5 - 5) * 72 / 62 - 0.5) * ONE) and bx == round(((0.5 - 7) * 104 / 92 - 0.5) * ONE)
    c = resync.crop_candidates((72, 104), (72, 104), [4, 5, 70], [7], [62, 63], [92, 200])
    assert c.dtype == np.int64 and c.shape == (4, 4)                          # top 70 and width 200 leave the canvas
    assert tuple(c[0]) == resync.warp_of_crop(4, 7, 62, 92, 72, 104) and tuple(c[3]) == resync.warp_of_crop(5, 7, 63, 92, 72, 104)
    assert resync.crop_candidates((72, 104), (72, 104), [80], [0], [8], [8]).shape == (0, 4)
