"""CPU-only: the rotated-leak entry points (ofmk_affine_units, ofmk_warp_affine_rgb8, ofmk_svd_affine_scores_rgb8,
ofmk_svd_detect_soft_affine_rgb8; build extensions) are exported, declared and bound, and refuse bad arguments with OFMK_E_ARG
before any HIP call, so these run without a GPU (the pointer values below are never dereferenced).  ofmk_affine_units is host
code: it is held against offmark.resync.affine_units and against the per-pixel statement of tests/_affine.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import _affine as af
import _warp as wp

E_ARG = -1
h, w, H, W, N, L, K = 61, 83, 72, 104, 3, 8, 5
IN, OUT, CANDS = 0x10000, 0x20000, 0x30000
SYMS = ("ofmk_affine_units", "ofmk_warp_affine_rgb8", "ofmk_svd_affine_scores_rgb8", "ofmk_svd_detect_soft_affine_rgb8")
ONE = 65536


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from offmark import _hip
    return _hip.load()


def scales(*v):
    return (C.c_double * 3)(*v)


def geom(ayy=ONE, ayx=0, by=0, axy=0, axx=ONE, bx=0):
    from offmark import _hip
    return C.byref(_hip.Affine(ayy, ayx, by, axy, axx, bx))


def null_geom():
    from offmark import _hip
    return C.cast(None, C.POINTER(_hip.Affine))


def refused(lib, rc):
    return rc == E_ARG and lib.ofmk_last_error().decode() != ""


def warp(lib, inp=IN, n=N, lh=h, lw=w, out=OUT, ho=H, wo=W, oy=0, ox=0, g=None, opts=None, **kw):
    g = geom(**kw) if g is None else g
    return refused(lib, lib.ofmk_warp_affine_rgb8(inp, n, lh, lw, out, ho, wo, oy, ox, g, None, opts))


def scores(lib, inp=IN, n=N, lh=h, lw=w, ch=H, cw=W, cands=CANDS, k=K, sc=None, blk=4, out=OUT, opts=None):
    sc = scales(0, 15, 0) if sc is None else sc
    return refused(lib, lib.ofmk_svd_affine_scores_rgb8(inp, n, lh, lw, ch, cw, cands, k, sc, blk, out, None, opts))


def readout(lib, inp=IN, n=N, lh=h, lw=w, ch=H, cw=W, g=None, l=L, sc=None, blk=4, out=OUT, opts=None, **kw):
    sc = scales(0, 15, 0) if sc is None else sc
    g = geom(**kw) if g is None else g
    return refused(lib, lib.ofmk_svd_detect_soft_affine_rgb8(inp, n, lh, lw, ch, cw, g, l, sc, blk, out, None, opts))


def units(lib, lh=h, lw=w, ch=H, cw=W, g=None, out=True, m=None, **kw):
    g = (geom(*m) if m is not None else geom(**kw)) if g is None else g
    r = (C.c_int * 5)(9, 9, 9, 9, 9)
    return lib.ofmk_affine_units(lh, lw, ch, cw, g, r if out else None), tuple(r)


def test_symbols_are_exported_declared_and_bound(lib):
    from offmark import _hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "offmark_hip.h")).read(), flags=re.S)
    for name in SYMS:
        assert hasattr(lib, name) and name in _hip.SIGNATURES and name in _hip.SYMBOLS
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert re.search(r"typedef\s+struct\s+ofmk_affine\s*\{\s*int64_t\s+ayy\s*,\s*ayx\s*,\s*by\s*,\s*axy\s*,\s*axx\s*,\s*bx\s*;\s*\}\s*ofmk_affine\s*;", header)
    assert re.search(r"\bint\s+ofmk_affine_units\s*\([^)]*const\s+ofmk_affine\s*\*\s*geom\s*,\s*int\s+out\[5\]\s*\)", header)
    for name in SYMS[1:]:
        assert re.search(r"\bint\s+" + name + r"\s*\(const\s+uint8_t\s*\*\s*in\s*,\s*int\s+n\s*,\s*int\s+h\s*,\s*int\s+w\s*,[^)]*const\s+ofmk_affine\s*\*[^)]*"
                         r"void\s*\*\s*stream\s*,\s*const\s+ofmk_opts\s*\*\s*opts\s*\)", header), name
    assert C.sizeof(_hip.Affine) == 48 and [f for f, _ in _hip.Affine._fields_] == ["ayy", "ayx", "by", "axy", "axx", "bx"]
    assert len(_hip.SIGNATURES["ofmk_affine_units"][1]) == 6 and len(_hip.SIGNATURES["ofmk_warp_affine_rgb8"][1]) == 12
    assert len(_hip.SIGNATURES["ofmk_svd_affine_scores_rgb8"][1]) == 13 == len(_hip.SIGNATURES["ofmk_svd_detect_soft_affine_rgb8"][1])
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
    assert call(lib, g=null_geom())
    for name in ("ayy", "ayx", "axy", "axx"):                                       # the four coefficients: [-2^20, 2^20]
        assert call(lib, **{name: (1 << 20) + 1}) and call(lib, **{name: -(1 << 20) - 1})
    assert call(lib, by=(1 << 48) + 1) and call(lib, bx=-(1 << 48) - 1) and call(lib, by=-(1 << 48) - 1) and call(lib, bx=(1 << 48) + 1)
    # the determinant: |ayy * axx - ayx * axy| >= 2^24
    assert call(lib, ayy=0) and call(lib, axx=0) and call(lib, ayy=(1 << 12) - 1, axx=1 << 12)
    assert call(lib, ayx=ONE, axy=ONE) and call(lib, ayy=ONE, ayx=ONE, axy=ONE, axx=ONE)      # singular
    assert call(lib, ayy=4096, ayx=1, axy=1, axx=4096)                                       # 2^24 - 1


def test_maps_at_the_ends_of_the_range_are_taken(lib):
    for kw in (dict(ayy=1 << 12, axx=1 << 12), dict(ayy=-(1 << 20), axx=1 << 20, ayx=1 << 20, axy=1 << 20), dict(axx=-ONE, bx=(w - 1) << 16),
               dict(ayy=0, ayx=ONE, axy=-ONE, axx=0, bx=1 << 48, by=-(1 << 48))):
        rc, _ = units(lib, **kw)
        assert rc == 0, (kw, lib.ofmk_last_error())


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
    assert units(lib, g=null_geom())[0] == E_ARG and units(lib, out=False)[0] == E_ARG
    assert units(lib, lh=0)[0] == E_ARG and units(lib, cw=0)[0] == E_ARG and units(lib, ayy=1 << 21)[0] == E_ARG
    assert units(lib, ayx=ONE, axy=ONE)[0] == E_ARG and units(lib, ch=1 << 14, cw=1 << 14)[0] == E_ARG


def check_units(lib, leak, canvas, m):
    from offmark import resync
    rc, got = units(lib, lh=leak[0], lw=leak[1], ch=canvas[0], cw=canvas[1], m=tuple(int(v) for v in m))
    assert rc == 0, (leak, canvas, m, lib.ofmk_last_error())
    mask = resync.affine_units(leak, canvas, m)
    assert np.array_equal(mask, af.units(leak, canvas, m)), (leak, canvas, m)
    assert got == af.rect_and_count(mask), (leak, canvas, m, got)
    return got


def test_units_equal_the_numpy_helper_and_the_per_pixel_statement(lib):
    from offmark import resync
    counts = set()
    for attack in af.ATTACKS:
        for m in af.candidate_geometries(attack):
            counts.add(check_units(lib, af.CANVAS, af.CANVAS, m)[4])
    assert min(counts) > 1
    # other leak sizes and canvases: a quarter turn, a flip, a shear, zooms, rotations about the centre of another leak size
    maps = [af.IDENTITY, af.hflip(83), (0, ONE, 0, -ONE, 0, 82 << 16), (ONE, 8192, 0, 0, ONE, 0), (-ONE, 0, 60 << 16, 0, -ONE, 82 << 16),
            (49152, 3000, -20000, -2500, 98304, 12345), (ONE, 0, 1 << 40, 0, ONE, 0), resync.affine_of_warp(wp.true_geometry((54, 80)))]
    maps += [resync.affine_of_rotation((72, 104), (61, 83), a, s) for a in (5.0, -17.0, 45.0, 180.0) for s in (1.0, 1.3)]
    seen = set()
    for leak in ((61, 83), (54, 80), (8, 8), (5, 6), (1, 1)):
        for canvas in ((72, 104), (8, 8), (7, 30), (100, 139)):
            for m in maps:
                seen.add(check_units(lib, leak, canvas, m)[4] > 0)
    assert seen == {True, False}
    assert units(lib, lh=72, lw=104)[1] == (0, 9, 0, 13, 117)                  # the identity on the uncropped frame: every unit
    assert units(lib, m=af.hflip(83))[1] == (0, 7, 0, 10, 70)                  # mirrored, the 61 x 83 leak fills the same 7 x 10 units
    assert units(lib, by=1 << 40)[1] == (0, 0, 0, 0, 0)                        # no unit
    assert units(lib, by=-(58 << 16), bx=-(90 << 16))[1] == (8, 9, 12, 13, 1)  # exactly one: canvas unit (8, 12)
