"""CPU-only: facts of the rotated-leak read-out on the NumPy statement (tests/_affine.py), on the oracle-marked recipe of
tests/_warp.py -- 3 segments x 4 frames of 72x104, copies (1, 0, 1) -- rotated about the frame centre with a float64 bilinear.  The
library is not involved: these pin what the fused calls are built to compute, and offmark.resync's host logic.  The last test
pins why no kernel reads RESCALED 4:2:0 planes."""
import numpy as np
import pytest

import _affine as af
import _planar_resync as pr
import _resync as rs
import _warp as wp

CANVAS = af.CANVAS


def test_zero_off_diagonals_are_the_axis_aligned_warp():
    from offmark import resync
    f = np.array(wp.leak("svd")[0])                                            # the zoomed recipe leak, 72 x 104
    for g4, out_hw, origin in ((wp.true_geometry(), CANVAS, (0, 0)), (wp.true_geometry(), (37, 45), (8, 16)),
                               ((49152, -8192, 98304, 16384), (85, 61), (0, 0))):
        g6 = resync.affine_of_warp(g4)
        assert g6 == (g4[0], 0, g4[1], 0, g4[2], g4[3])
        got, inside = af.warp(f, g6, out_hw, origin)
        ref, ref_inside = wp.warp(f, g4, out_hw, origin)
        assert np.array_equal(got, ref) and np.array_equal(inside, ref_inside) and ref.any()
        mask = af.units(f.shape[:2], CANVAS, g6)
        i0, i1, j0, j1 = wp.units(f.shape[:2], CANVAS, g4)
        assert af.rect_and_count(mask) == (i0, i1, j0, j1, (i1 - i0) * (j1 - j0))


def test_the_horizontal_flip_and_a_quarter_turn_move_whole_pixels():
    f = np.array(rs.oracle_leak()[0])                                          # 61 x 83
    h, w = f.shape[:2]
    out, inside = af.warp(f, af.hflip(w), (h, w))
    assert inside.all() and np.array_equal(out, f[:, ::-1])
    out, inside = af.warp(f, (0, af.ONE, 0, -af.ONE, 0, (w - 1) << 16), (w, h))       # canvas (y, x) reads leak (x, w - 1 - y)
    assert inside.all() and np.array_equal(out, np.rot90(f, 1))


@pytest.mark.parametrize("attack", list(af.ATTACKS))
def test_the_corner_rule_is_the_per_pixel_rule(attack):
    from offmark import resync
    cands = af.candidate_geometries(attack)
    assert cands.shape == (35, 6) and len({tuple(c) for c in cands}) == 35
    counts = []
    for g in cands:
        mask = af.units(CANVAS, CANVAS, g)
        assert np.array_equal(mask, af.corner_units(CANVAS, CANVAS, g))
        assert np.array_equal(mask, resync.affine_units(CANVAS, CANVAS, g))
        counts.append(int(mask.sum()))
    if attack == "2deg":
        mask = af.units(CANVAS, CANVAS, cands[0])
        assert counts[0] == 101 and af.rect_and_count(mask)[:4] == (0, 9, 0, 13)       # 101 of 117: convex, not a rectangle
        assert all(np.ptp(np.flatnonzero(r)) + 1 == r.sum() for r in mask if r.any())    # every row of units is one run
    assert min(counts) > 0


def test_affine_of_warp_and_affine_of_rotation():
    from offmark import resync
    assert resync.affine_of_warp(wp.IDENTITY) == af.IDENTITY == resync.affine_of_rotation(CANVAS, CANVAS, 0.0)
    g4 = wp.true_geometry()
    g6 = resync.affine_of_warp(g4)
    assert (g6[0], g6[2], g6[4], g6[5]) == tuple(g4) and g6[1] == g6[3] == 0
    ayy, ayx, by, axy, axx, bx = resync.affine_of_rotation(CANVAS, CANVAS, 2.0)
    c, s = np.cos(np.deg2rad(2.0)), np.sin(np.deg2rad(2.0))
    assert (ayy, ayx, axy, axx) == tuple(int(np.rint(v * 65536)) for v in (c, s, -s, c))
    assert by == int(np.rint((35.5 - c * 35.5 - s * 51.5) * 65536)) and bx == int(np.rint((51.5 + s * 35.5 - c * 51.5) * 65536))
    # a shift of the canvas by whole pixels at angle 0 is a whole-pixel b; a quarter turn swaps the axes
    assert resync.affine_of_rotation(CANVAS, CANVAS, 0.0, shift=(3, -5)) == (af.ONE, 0, -3 << 16, 0, af.ONE, 5 << 16)
    assert resync.affine_of_rotation((8, 8), (8, 8), 90.0) == (0, af.ONE, 0, -af.ONE, 0, 7 << 16)
    k = resync.rotation_candidates(CANVAS, CANVAS, [1.0, 2.0], [1.0, 1e-6], [0.0], [0.0, 1.0])
    assert k.dtype == np.int64 and k.shape == (4, 6)                           # scale 1e-6 is out of the map's range
    assert tuple(k[3]) == resync.affine_of_rotation(CANVAS, CANVAS, 2.0, 1.0, (0.0, 1.0))
    with pytest.raises(ValueError):
        resync.affine_units(CANVAS, CANVAS, (1, 0, 0, 0, 1, 0))                # determinant below 2^24


@pytest.mark.parametrize("attack", list(af.ATTACKS))
def test_the_true_geometry_ranks_first_the_copies_are_read_and_unmarked_content_has_less_contrast(attack):
    """Measured with this statement (the first 4 frames, normalised = score / (2^14 * units * frames)), printed by the test:
    2 degrees: marked true 0.7954 / best other 0.6897 (contrast 1.153), unmarked contrast 0.938 (true / best other);
    -3 degrees with step 1.10: marked 0.7712 / 0.6726 (1.147), unmarked 0.954.  The assertions are the orderings only."""
    from offmark import resync
    cands = af.candidate_geometries(attack)
    dec = af.StatementDecoder()
    got = {}
    for codec in ("svd", "none"):
        scores = dec.affine_scores_u8(af.leak(codec, attack)[:af.SEARCH_FRAMES], CANVAS, cands)
        got[codec] = resync.best_geometry(scores, cands, CANVAS, CANVAS)
        n = got[codec]["normalised"]
        print(f"{attack} {codec}: index {got[codec]['index']} true {n[0]:.4f} best other {np.delete(n, 0).max():.4f} "
              f"true / best other {n[0] / np.delete(n, 0).max():.4f} contrast {got[codec]['contrast']:.4f}")
    marked, unmarked = got["svd"], got["none"]
    assert marked["index"] == 0 and marked["geometry"] == tuple(cands[0]) and marked["contrast"] > 1.0
    assert unmarked["index"] != 0                                              # on unmarked content the true geometry is not first
    un = unmarked["normalised"]
    assert un[0] / np.delete(un, 0).max() < marked["contrast"]
    out = resync.read_rescaled_leak(dec, af.leak("svd", attack), rs.recipe_segments(), CANVAS, rs.recipe_candidates(), cands, key=af.KEY,
                                    L=af.L8, search_frames=af.SEARCH_FRAMES)
    assert out["index"] == 0 and out["geometry"] == tuple(cands[0]) and out["contrast"] == marked["contrast"]
    assert list(out["picks"]) == list(af.CHOSEN) and not out["ambiguous"] and out["base"] == 0 and out["runner_up_score"] is None


def test_four_column_lists_read_as_before_and_the_dct_decoder_has_no_affine_read_out():
    from offmark import resync
    g4 = wp.candidate_geometries()[:1]
    dec = wp.StatementDecoder("svd", search=False)
    out = resync.read_rescaled_leak(dec, wp.leak("svd"), rs.recipe_segments(), CANVAS, rs.recipe_candidates(), g4, key=wp.KEY, L=wp.L8)
    assert list(out["picks"]) == list(wp.CHOSEN) and out["geometry"] == tuple(g4[0])
    with pytest.raises(ValueError, match="affine"):                            # this decoder has decode_soft_warp_u8 only, as DctDecoder
        resync.read_rescaled_leak(dec, wp.leak("svd"), rs.recipe_segments(), CANVAS, rs.recipe_candidates(), [resync.affine_of_warp(g4[0])])
    b = resync.best_geometry(np.array([[16384 * 117, 5]]), np.array([af.IDENTITY, (af.ONE, 0, 1 << 40, 0, af.ONE, 0)]), CANVAS, CANVAS)
    assert b["index"] == 0 and b["normalised"][0] == 1.0 and b["normalised"][1] == 0 and b["geometry"] == af.IDENTITY


# ---- why no kernel reads rescaled 4:2:0 planes ------------------------------------------------------------------------------------
PLANAR_CASES = {"odd-crop-zoom-back": ((5, 7, 62, 92), (72, 104)), "even-crop-zoom-back": ((6, 8, 62, 92), (72, 104)),
                "even-crop-down": ((4, 8, 64, 88), (54, 80))}


@pytest.mark.parametrize("case", list(PLANAR_CASES))
def test_rescaled_planes_lose_the_mark(case):
    """The planar-marked recipe converted to RGB, cropped, resized (tests/_warp.py: resize), converted to 4:2:0 planes -- the leak --
    and read back through RGB with the integer warp: the true geometry does not rank first among its 49 neighbours, and the
    units' signs agree with the marked frame's far less than a read-out needs.  A unit's mark lives in 4x4 chroma samples; two
    bilinear resamplings at chroma resolution destroy it.  Measured (printed): sign agreement 0.58-0.63, true / best other
    0.92-0.94."""
    from offmark import resync
    crop, leak_hw = PLANAR_CASES[case]
    marked = [pr.to_rgb(p) for p in pr.marked_planes("svd")[:af.SEARCH_FRAMES]]
    leak = [pr.to_rgb(pr.to_planes(wp.resize(f[crop[0]:crop[0] + crop[2], crop[1]:crop[1] + crop[3]], leak_hw))) for f in marked]
    top, left, ch, cw = crop
    d = [(a, b) for a in range(-2, 3) for b in range(-2, 3) if (a, b) != (0, 0)]
    crops = [crop] + [(top + a, left + b, ch, cw) for a, b in d] + [(top, left, ch + a, cw + b) for a, b in d] + [(top + 1, left + 1, ch - 2, cw - 2)]
    cands = np.asarray([resync.warp_of_crop(*c, *leak_hw) for c in crops], dtype=np.int64)
    scores = np.asarray([[wp.statement_score(f, CANVAS, g) for g in cands] for f in leak], dtype=np.int64)
    found = resync.best_geometry(scores, cands, leak_hw, CANVAS)
    n = found["normalised"]
    agree, total = 0, 0
    for f, ref in zip(leak, marked):
        m, (i0, i1, j0, j1) = wp.unit_metrics(f, CANVAS, cands[0])
        want = wp.ss.statement(np.ascontiguousarray(ref[8 * i0:8 * i1, 8 * j0:8 * j1]))["m"]
        agree += int((np.sign(m) == np.sign(want)).sum())
        total += m.size
    print(f"{case}: index {found['index']} true {n[0]:.4f} best other {np.delete(n, 0).max():.4f} true / best other "
          f"{n[0] / np.delete(n, 0).max():.4f} sign agreement {agree / total:.3f} over {total} units")
    assert found["index"] != 0
    assert agree / total < 0.8
