"""GPU: the warped read-out kernels at the edges of their fixed-point range (engine.warp / warp_affine, the fused svd_*_scores and
svd_detect_soft_* calls, svd_affine_phase_scores, align_sums, align_residuals; build extensions, not reference semantics).

The maps are tests/_geometry_edges.py's seeded families: coefficients at +-2^20 in every sign pattern, determinants at 2^24,
positions exactly where the inside rule flips, offsets near 2^33 with sample indices in the thousands, leaks 1 to 3 px wide or
high.  test_geometry_edges_statement.py holds, on the CPU, that these maps have counting units, units that do not count and pixels on
both sides of every edge.  Here every call is held against the oracle its own test file uses -- the NumPy statements of
tests/_affine.py, _warp.py, _align.py and _temporal.py, and for the fused calls the chain they replace (the per-pixel int64 warp on
the device, svd_detect_soft, the statement's per-pixel units) -- integer for integer, nothing masked out; output buffers arrive
filled with garbage.  Two identities need no statement: a map composed with a left-right flip reads the mirrored leak alike, and a
map composed with a whole-pixel canvas shift is the phase call's entry."""
import numpy as np
import pytest

import _affine as af
import _align as al
import _geometry_edges as ge
import _temporal as tp
import _warp as wp

pytestmark = pytest.mark.gpu

N = 2
READ_OUT_LENGTHS = (7, 64)                   # 7 divides none of the unit counts here (17 x 25, 9 x 13, 2 x 1025)


@pytest.fixture(scope="module")
def eng():
    import torch
    from offmark.engine import DctEngine
    torch.cuda.set_device(0)
    return DctEngine()


@pytest.fixture(scope="module")
def leaks():
    """leaks(hw) -> (host u8 [2, h, w, 3] noise, the same on the device), made once per size."""
    import torch
    made = {}

    def get(hw):
        if hw not in made:
            host = ge.noise((N, *hw, 3), 30, *hw)
            made[hw] = (host, torch.from_numpy(np.array(host)).cuda())
        return made[hw]

    return get


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def garbage(shape, dtype=None):
    """The output buffer a call gets holds anything: the library writes or clears all of it."""
    import torch
    if dtype is torch.uint8:
        return torch.full(shape, 0x5A, dtype=torch.uint8, device="cuda")
    return torch.full(shape, 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")


def six(g4):
    ay, by, ax, bx = g4
    return ay, 0, by, 0, ax, bx


interleaved = ge.interleaved


# (leak, canvas, maps) of every affine family, at most 64 maps each
FAMILIES = {
    "steepest-a": (ge.STEEP_LEAK, ge.CANVAS, ge.steepest(64)[:32]),           # the 64 maps in two cases of 32: each stays quick
    "steepest-b": (ge.STEEP_LEAK, ge.CANVAS, ge.steepest(64)[32:]),
    "uniform-a": (ge.STEEP_LEAK, ge.CANVAS, ge.uniform(64)[:32]),
    "uniform-b": (ge.STEEP_LEAK, ge.CANVAS, ge.uniform(64)[32:]),
    "smallest-determinant": (ge.ODD_LEAK, ge.CANVAS, ge.smallest_determinant(32)),
    "anisotropic": (ge.STEEP_LEAK, ge.CANVAS, ge.anisotropic(16)),
    "boundary": (ge.ODD_LEAK, ge.SMALL_CANVAS, ge.boundary(ge.ODD_LEAK)),
    "far-wide": (ge.WIDE_LEAK, ge.LONG_CANVAS, ge.far(ge.WIDE_LEAK)),
    "far-tall": (ge.TALL_LEAK, ge.LONG_CANVAS, ge.far(ge.TALL_LEAK)),
    **{f"tiny-{h}x{w}": ((h, w), ge.SMALL_CANVAS, ge.tiny((h, w))) for h, w in ge.TINY_LEAKS},
}
PIXEL_FAMILIES = {                           # for the per-pixel calls: nothing needs a whole unit inside
    **FAMILIES,
    **{f"boundary-{h}x{w}": ((h, w), ge.SMALL_CANVAS, ge.boundary((h, w))) for h, w in ((1, 83), (61, 2), (3, 3))},
}
AXIS_FAMILIES = {
    "axis-steep": (ge.STEEP_LEAK, ge.CANVAS, ge.axis_aligned()),
    "axis-odd": (ge.ODD_LEAK, ge.CANVAS, ge.axis_aligned(ge.ODD_LEAK)),
    "axis-far": (ge.WIDE_LEAK, ge.LONG_CANVAS, ge.axis_aligned_far()),
}


def windows(family, canvas):
    """The whole canvas, and a window with a non-zero origin that holds both pixels the maps are anchored at (the canvas centre and
    ge.tile_corner); the far families through ``origin`` instead of the long canvas."""
    if "far" in family:
        return ((16, 264), (0, ge.FAR_X - 140)), ((9, 77), (5, ge.FAR_X - 30))
    return (canvas, (0, 0)), ((85, 53), (canvas[0] // 2 - 21, canvas[1] // 2 - 21))


# ---- 1. the two warps against their statements ------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", PIXEL_FAMILIES)
def test_warp_affine_equals_the_statement(eng, leaks, family):
    import torch
    leak, canvas, maps = PIXEL_FAMILIES[family]
    host, dev = leaks(leak)
    lit = 0
    maps = maps[:32:2] if "far" in family else maps[:32]                       # a statement warp of the long leaks is slow: four far maps
    for k, g in enumerate(maps):
        for out_hw, origin in windows(family, canvas)[:1 if k % 4 and "far" not in family else 2]:      # the window: every fourth map
            got = eng.warp_affine(dev, g, out_hw, origin=origin, out=garbage((N, *out_hw, 3), torch.uint8)).cpu().numpy()
            ref = np.stack([af.warp(f, g, out_hw, origin)[0] for f in host])
            assert got.shape == ref.shape and got.dtype == np.uint8 and np.array_equal(got, ref), (g, origin, np.argwhere(got != ref)[:5])
            lit += bool(ref.any())
    assert lit >= len(maps)                                                    # every map lights pixels in a window


def test_the_far_warp_over_the_whole_long_canvas(eng, leaks):
    """16 x 8200 output pixels: the first 5000 columns and more read far outside the leak, at positions down to -95 000 px; in the
    lit columns the sample indices pass 32768, where a Q16 position no longer fits 32 bits."""
    import torch
    for leak in (ge.WIDE_LEAK, ge.TALL_LEAK):
        host, dev = leaks(leak)
        for g in ge.far(leak)[::3]:
            got = eng.warp_affine(dev, g, ge.LONG_CANVAS, out=garbage((N, *ge.LONG_CANVAS, 3), torch.uint8)).cpu().numpy()
            ref = np.stack([af.warp(f, g, ge.LONG_CANVAS)[0] for f in host])
            assert np.array_equal(got, ref) and ref[:, :, 8000:].any() and not ref[:, :, :5000].any()


@pytest.mark.parametrize("family", AXIS_FAMILIES)
def test_warp_equals_the_statement(eng, leaks, family):
    import torch
    leak, canvas, maps = AXIS_FAMILIES[family]
    host, dev = leaks(leak)
    for g in maps:
        for out_hw, origin in windows(family, canvas):
            got = eng.warp(dev, g, out_hw, origin=origin, out=garbage((N, *out_hw, 3), torch.uint8)).cpu().numpy()
            ref = np.stack([wp.warp(f, g, out_hw, origin)[0] for f in host])
            assert np.array_equal(got, ref), (g, origin, np.argwhere(got != ref)[:5])
    whole = eng.warp(dev, maps[-1], canvas).cpu().numpy()
    assert whole.any() and np.array_equal(whole, eng.warp_affine(dev, six(maps[-1]), canvas).cpu().numpy())


# ---- 2. the fused scores and read-outs against the chain ----------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_affine_scores_and_read_out_equal_the_chain(eng, leaks, family):
    leak, canvas, maps = FAMILIES[family]
    _, dev = leaks(leak)
    cands, good, bad = interleaved(maps, ge.out_of_range())
    got = eng.svd_affine_scores(dev, canvas, np.array(cands, np.int64), scores=garbage((N, len(cands)))).cpu().numpy()
    assert got.shape == (N, len(cands)) and got.dtype == np.int64
    chain = {k: af.chain_unit_metrics(eng, dev, canvas, cands[k]) for k in good}
    ref = np.zeros_like(got)
    for k in good:
        ref[:, k] = np.abs(chain[k]).sum(axis=(1, 2))
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    assert not got[:, bad].any()                                               # out of range: zeros ...
    alone = eng.svd_affine_scores(dev, canvas, np.array([cands[k] for k in good], np.int64)).cpu().numpy()
    assert np.array_equal(alone, got[:, good])                                 # ... and the neighbours do not change
    counting = [k for k in good if ref[:, k].all()]
    assert len(counting) >= (len(maps) // 2 if family.startswith("tiny") else len(maps)), len(counting)
    # the read-out at a length that does not divide the unit count, and at 64
    for k in counting[:3] + counting[-3:]:
        for L in READ_OUT_LENGTHS:
            soft = eng.svd_detect_soft_affine(dev, canvas, cands[k], L, soft=garbage((N, L))).cpu().numpy()
            want = np.stack([af.ss.regroup(f.reshape(-1), L) for f in chain[k]])
            assert soft.shape == (N, L) and np.array_equal(soft, want) and want.any(), (cands[k], L)


@pytest.mark.parametrize("family", AXIS_FAMILIES)
def test_warp_scores_and_read_out_equal_the_chain(eng, leaks, family):
    """The axis-aligned kernels keep the previous canvas row's two leak rows: at 2^20 per row neither is ever kept, at 2^12 both
    repeat over 16 canvas rows of a leak that is taller than one pixel."""
    leak, canvas, maps = AXIS_FAMILIES[family]
    _, dev = leaks(leak)
    H8, W8 = canvas[0] // 8, canvas[1] // 8
    cands, good, bad = interleaved(maps, ge.out_of_range4())
    got = eng.svd_warp_scores(dev, canvas, np.array(cands, np.int64), scores=garbage((N, len(cands)))).cpu().numpy()
    chain = {}
    for k in good:
        i0, i1, j0, j1 = wp.units(leak, canvas, cands[k])                      # the statement's counting rectangle, per pixel
        mask = np.zeros((H8, W8), bool)
        mask[i0:i1, j0:j1] = True
        m = eng.svd_detect_soft(eng.warp(dev, cands[k], (8 * H8, 8 * W8)), H8 * W8).cpu().numpy().reshape(-1, H8, W8)
        chain[k] = np.where(mask[None], m, 0)
    ref = np.zeros_like(got)
    for k in good:
        ref[:, k] = np.abs(chain[k]).sum(axis=(1, 2))
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    assert not got[:, bad].any()
    assert np.array_equal(eng.svd_warp_scores(dev, canvas, np.array([cands[k] for k in good], np.int64)).cpu().numpy(), got[:, good])
    assert np.array_equal(eng.svd_affine_scores(dev, canvas, np.array([six(cands[k]) for k in good], np.int64)).cpu().numpy(), got[:, good])
    counting = [k for k in good if ref[:, k].all()]
    assert len(counting) >= (len(maps) if family != "axis-odd" else 16), len(counting)
    for k in counting[:3] + counting[-3:]:
        for L in READ_OUT_LENGTHS:
            soft = eng.svd_detect_soft_warp(dev, canvas, cands[k], L, soft=garbage((N, L))).cpu().numpy()
            want = np.stack([af.ss.regroup(f.reshape(-1), L) for f in chain[k]])
            assert np.array_equal(soft, want) and want.any(), (cands[k], L)


# ---- 3. the dense shift search ------------------------------------------------------------------------------------------------------
PHASE_FAMILIES = {                           # the far maps on a shorter canvas, |b| above 2^31: 64 statement warps of it stay quick
    **FAMILIES,
    "far-wide": (ge.PHASE_WIDE_LEAK, ge.PHASE_LONG_CANVAS, ge.far(ge.PHASE_WIDE_LEAK, ge.PHASE_LONG_CANVAS, ge.PHASE_FAR_X)),
    "far-tall": (ge.PHASE_TALL_LEAK, ge.PHASE_LONG_CANVAS, ge.far(ge.PHASE_TALL_LEAK, ge.PHASE_LONG_CANVAS, ge.PHASE_FAR_X)),
}
# a map (with two out-of-range neighbours) per case: the reference takes 64 statement warps per map
PHASE_CASES = [(f, k) for f, ks in (("steepest-a", ge.PHASE_STEEPEST + (0, 6)), ("uniform-a", (0, 1, 2, 3)), ("smallest-determinant", (0, 5)),
                                    ("anisotropic", (0, 1, 2, 3)), ("boundary", (0, 11, 22, 33, 44, 55)), ("far-wide", (1, 6)), ("far-tall", (2, 5)),
                                    ("tiny-2x3", (0, 6, 12)), ("tiny-1x83", (3, 9, 15))) for k in ks]


@pytest.mark.parametrize("case", PHASE_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_phase_scores_and_units_equal_the_64_shifted_maps(eng, leaks, case):
    """Entry [f][k][8 py + px] is svd_affine_scores under the map composed with the whole-pixel canvas shift (py, px) -- an identity
    between two device calls --, and units[k][8 py + px] the statement's per-pixel count of that shifted map."""
    from offmark import resync
    family, pick = case
    leak, canvas, maps = PHASE_FAMILIES[family]
    _, dev = leaks(leak)
    cands, good, bad = interleaved(maps[pick:pick + 1], ge.out_of_range()[:2])
    K = len(cands)
    cands = np.array(cands, np.int64)
    scores, units = eng.svd_affine_phase_scores(dev, canvas, cands, scores=garbage((N, K, 64)), units=garbage((K, 64)))
    got, got_units = scores.cpu().numpy(), units.cpu().numpy()
    shifted = np.stack([resync.shift_affine(cands, py, px) for py in range(8) for px in range(8)], axis=1)      # [K, 64, 6]
    ref = eng.svd_affine_scores(dev, canvas, shifted.reshape(K * 64, 6)).cpu().numpy().reshape(N, K, 64)
    ref[:, bad] = 0
    ref_units = np.zeros((K, 64), np.int64)
    for k in good:
        ref_units[k] = [af.units(leak, canvas, g).sum() for g in shifted[k]]
    assert np.array_equal(got_units, ref_units), np.argwhere(got_units != ref_units)[:5]
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    assert ((got > 0) == (ref_units > 0)[None]).all() and not got[:, bad].any() and not got_units[bad].any()
    assert ref_units[good].any(axis=1).all()
    # the count depends on the shift, except at 16 x magnification, where the whole canvas stays inside the leak
    assert len({int(u) for u in ref_units[good].reshape(-1)}) > 1 or family == "smallest-determinant"


# ---- 4. the registration sums and the residuals ---------------------------------------------------------------------------------------
ALIGN_CASES = ge.ALIGN_CASES                # shared with test_gpu_value_edges.py


@pytest.mark.parametrize("case", ALIGN_CASES)
def test_align_sums_equal_the_statement(eng, leaks, case):
    leak, canvas, maps = ALIGN_CASES[case]
    assert len(maps) <= 16
    host, dev = leaks(leak)
    sources = ge.noise((N, *canvas, 3), 40, *canvas)
    cands, good, bad = interleaved(maps, ge.out_of_range()[4:])
    got = eng.align_sums(cuda(sources), dev, np.array(cands, np.int64), sums=garbage((N, len(cands), 29))).cpu().numpy()
    want = al.statement_sums(sources, host, cands)
    assert got.shape == want.shape == (N, len(cands), 29)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert not want[:, bad].any() and want[:, good, 28].all() and (want[:, good, 27] > 0).all()


RESIDUAL_MAPS = ge.RESIDUAL_MAPS


@pytest.mark.parametrize("span", [1, 16])
@pytest.mark.parametrize("which", RESIDUAL_MAPS, ids=lambda c: f"{c[0]}-{c[1]}")
def test_align_residuals_equal_the_statement(eng, leaks, which, span):
    """A library of 12 frames; at span 16 the windows -3 .. 12 and 5 .. 20 leave it at either end."""
    first = np.array([-3, 5] if span == 16 else [0, 11], np.int32)
    case, k = which
    leak, canvas, maps = ALIGN_CASES[case]
    host, dev = leaks(leak)
    library = ge.noise((12, *canvas, 3), 50, *canvas)
    buf = garbage((N, span, 2))
    got = eng.align_residuals(cuda(library), dev, first, span, maps[k], out=buf)
    assert got is buf
    got, want = got.cpu().numpy(), tp.residuals(library, host, first, span, maps[k])
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    inside = want[:, :, 1] > 0
    if span == 16:
        assert not inside[0, :3].any() and inside[0, 3:15].all() and not inside[0, 15:].any() and inside[1, :7].all() and not inside[1, 7:].any()
    else:
        assert inside.all() and want[:, :, 0].all()


# ---- 5. the mirror identity -------------------------------------------------------------------------------------------------------------
# Steep maps in multiples of 256 (the weights then mirror exactly), none with a pixel in the leak's last-column fraction: the flipped
# map on the mirrored leak gives the same warp, scores, read-outs, sums and residuals as the map on the leak.
@pytest.fixture(scope="module")
def mirror(leaks):
    import torch
    _, dev = leaks(ge.STEEP_LEAK)
    pairs = ge.mirror_pairs(8)
    return (dev, torch.flip(dev, dims=[2]).contiguous(), pairs, np.array([p[0] for p in pairs], np.int64), np.array([p[1] for p in pairs], np.int64))


def test_a_flipped_map_scores_and_reads_the_mirrored_leak_alike(eng, mirror):
    import torch
    dev, flipped, pairs, gs, ms = mirror
    a, b = eng.svd_affine_scores(dev, ge.CANVAS, gs, scores=garbage((N, 8))), eng.svd_affine_scores(flipped, ge.CANVAS, ms, scores=garbage((N, 8)))
    assert torch.equal(a, b) and bool(a.all())
    for g, m in pairs[:3]:
        for L in READ_OUT_LENGTHS:
            a = eng.svd_detect_soft_affine(dev, ge.CANVAS, g, L)
            assert torch.equal(a, eng.svd_detect_soft_affine(flipped, ge.CANVAS, m, L)) and bool(a.any())
        assert torch.equal(eng.warp_affine(dev, g, ge.CANVAS), eng.warp_affine(flipped, m, ge.CANVAS))


def test_a_flipped_map_has_the_sums_and_residuals_of_the_mirrored_leak(eng, mirror):
    import torch
    dev, flipped, pairs, gs, ms = mirror
    sources = cuda(ge.noise((N, *ge.CANVAS, 3), 40, *ge.CANVAS))
    a, b = eng.align_sums(sources, dev, gs, sums=garbage((N, 8, 29))), eng.align_sums(sources, flipped, ms, sums=garbage((N, 8, 29)))
    assert torch.equal(a, b) and bool(a[:, :, 28].all())
    first = np.array([0, 1], np.int32)
    for g, m in pairs[:3]:
        a = eng.align_residuals(sources, dev, first, 2, g)
        assert torch.equal(a, eng.align_residuals(sources, flipped, first, 2, m)) and bool(a[0].all()) and not bool(a[1, 1].any())


def test_a_flipped_map_has_the_unshifted_phase_entry_of_the_mirrored_leak(eng, mirror):
    import torch
    dev, flipped, pairs, gs, ms = mirror
    pa, ua = eng.svd_affine_phase_scores(dev, ge.CANVAS, gs[:3])
    pb, ub = eng.svd_affine_phase_scores(flipped, ge.CANVAS, ms[:3])
    assert torch.equal(ua[:, 0], ub[:, 0]) and torch.equal(pa[:, :, 0], pb[:, :, 0]) and bool(pa[:, :, 0].all())
    assert torch.equal(pa[:, :, 0], eng.svd_affine_scores(dev, ge.CANVAS, gs[:3]))
