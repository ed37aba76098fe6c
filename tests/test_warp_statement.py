"""CPU-only: facts of the rescaled-leak read-out on the NumPy statement (tests/_warp.py), on the oracle-marked recipe -- 3 segments x 4
frames of 72x104, copies (1, 0, 1), cropped to rows 5:67 / columns 7:99 and resized back to 72x104 with a float64 bilinear.  The
library is not involved: these pin what the fused calls are built to compute, and offmark.resync's host logic."""
import numpy as np
import pytest

import _resync as rs
import _warp as wp

CANVAS = (wp.H, wp.W)


def test_the_statement_warp_at_the_identity_and_at_a_shift():
    f = np.array(rs.oracle_leak()[0])                                          # 61 x 83
    out, inside = wp.warp(f, wp.IDENTITY, f.shape[:2])
    assert inside.all() and np.array_equal(out, f)
    out, inside = wp.warp(f, (65536, 3 << 16, 65536, -(5 << 16)), (70, 90))     # canvas (y, x) reads leak (y + 3, x - 5)
    assert np.array_equal(out[:58, 5:88], f[3:, :]) and inside[:58, 5:88].all()
    assert not inside[58:].any() and not inside[:, :5].any() and not inside[:, 88:].any() and not out[~inside].any()


def test_the_true_geometry_ranks_first_and_above_unmarked_content():
    """Measured with this statement (DwtDctSvd, the first 4 frames, normalised = score / (2^14 * units * frames), 77 counting units):
    marked leak: true geometry 0.8020, best of the 49 others 0.6819, contrast 1.176; unmarked sources attacked the same way: at
    most 0.6732 over all 50 candidates (0.6178 at the true geometry, contrast 1.011).  The same leak scaled down to 54x80: 0.7346
    against 0.6701 (contrast 1.096), unmarked at most 0.6676.  The bounds below are facts of the recipe, not tolerances: the true
    geometry is first, and its score exceeds every unmarked score."""
    from offmark import resync
    cands = wp.candidate_geometries()
    assert cands.shape == (50, 4) and len({tuple(c) for c in cands}) == 50
    assert resync.warp_units(wp.ZOOM_HW, CANVAS, cands[0]) == (1, 8, 1, 12)
    dec = wp.StatementDecoder("svd")
    got = {}
    for codec in ("svd", "none"):
        scores = dec.warp_scores_u8(wp.leak(codec)[:wp.SEARCH_FRAMES], CANVAS, cands)
        got[codec] = resync.best_geometry(scores, cands, wp.ZOOM_HW, CANVAS)
        n = got[codec]["normalised"]
        print(f"{codec}: index {got[codec]['index']} true {n[0]:.4f} best other {np.delete(n, 0).max():.4f} contrast {got[codec]['contrast']:.4f}")
    marked, unmarked = got["svd"], got["none"]
    assert marked["index"] == 0 and marked["geometry"] == tuple(cands[0])
    assert marked["normalised"][0] > unmarked["normalised"].max()
    assert marked["contrast"] == pytest.approx(marked["normalised"][0] / np.delete(marked["normalised"], 0).max())


@pytest.mark.parametrize("codec", ["svd", "dct"])
def test_the_host_logic_reads_the_copies_at_the_true_geometry(codec):
    from offmark import resync
    geoms = wp.candidate_geometries()[:1]
    out = resync.read_rescaled_leak(wp.StatementDecoder(codec, search=False), wp.leak(codec), rs.recipe_segments(), CANVAS,
                                    rs.recipe_candidates(), geoms, key=wp.KEY, L=wp.L8)
    assert list(out["picks"]) == list(wp.CHOSEN) and not out["ambiguous"] and out["base"] == 0
    assert out["geometry"] == tuple(geoms[0]) and out["contrast"] is None and out["runner_up_score"] is None
    assert out["soft_by_segment"].shape == (wp.S, wp.L8) and out["segments"] == [0, 1, 2]


def test_a_search_needs_a_decoder_that_has_one():
    from offmark import resync
    with pytest.raises(ValueError, match="no geometry search"):
        resync.read_rescaled_leak(wp.StatementDecoder("dct", search=False), wp.leak("dct"), rs.recipe_segments(), CANVAS,
                                  rs.recipe_candidates(), wp.candidate_geometries()[:2])


def test_the_search_and_the_read_out_end_to_end_on_the_statement():
    from offmark import resync
    out = resync.read_rescaled_leak(wp.StatementDecoder("svd"), wp.leak("svd"), rs.recipe_segments(), CANVAS, rs.recipe_candidates(),
                                    wp.candidate_geometries(), key=wp.KEY, L=wp.L8, search_frames=wp.SEARCH_FRAMES)
    assert out["index"] == 0 and list(out["picks"]) == list(wp.CHOSEN) and out["contrast"] > 1.0


def test_best_geometry_excludes_candidates_without_a_unit():
    from offmark import resync
    cands = np.array([wp.IDENTITY, (65536, 1 << 40, 65536, 0), (65536, -(11 << 16), 65536, -(21 << 16))], np.int64)
    g = resync.best_geometry(np.array([[5 * 16384 * 70, 999, 16384 * 35]]), cands, (61, 83), CANVAS)       # 70, 0 and 70 units
    assert g["index"] == 0 and g["normalised"][1] == 0 and g["normalised"][0] == 5.0 and g["contrast"] == 10.0
    with pytest.raises(ValueError):
        resync.best_geometry(np.array([[1]]), cands[1:2], (61, 83), CANVAS)


def test_align_segments_keeps_its_results_and_takes_a_fixed_rotation():
    from offmark import resync
    rng = np.random.default_rng(3)
    soft = rng.integers(-50000, 50000, (3, 8))
    full = resync.align_segments(soft, rs.recipe_candidates(), wp.KEY)
    assert all(np.array_equal(full[k], v) for k, v in resync.align_segments(soft, rs.recipe_candidates(), wp.KEY, bases=range(8)).items())
    fixed = resync.align_segments(soft, rs.recipe_candidates(), wp.KEY, bases=(full["base"],))
    assert fixed["base"] == full["base"] and np.array_equal(fixed["picks"], full["picks"]) and fixed["score"] == full["score"]
    assert fixed["runner_up_score"] is None
