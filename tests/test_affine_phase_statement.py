"""CPU-only: facts of the dense shift search on the NumPy statement (tests/_affine_phase.py), on the oracle-marked recipe of
tests/_warp.py rotated by 2 degrees (tests/_affine.py) and then CROPPED off-centre, so that the translation is unknown.  The library
is not involved: these pin what ofmk_svd_affine_phase_scores_rgb8 is built to compute and offmark.resync's host logic
(shift_affine, subpixel_shifts, best_shifted_geometry, read_transformed_leak).

Measured with this statement on the first 4 frames (normalised = score / (2^14 * units * frames); printed by the tests):
  leak A (rows 7:63, columns 5:95): truth 0.740 at phase (1, 2), 65 units; its second phase 0.677; every other candidate <= 0.706;
  leak B (rows 7:64, columns 5:96): truth (sub-pixel shift (0.5, 0.5)) 0.742 at phase (1, 2), 73 units; its second phase 0.690;
  every other candidate <= 0.695; with whole-pixel shifts only the best entry is 0.691, the unmarked level, and the copies are wrong.
The contrasts are thin (about 1.05 between candidates, 1.07-1.09 between phases), so the assertions are rankings and copies."""
import numpy as np
import pytest

import _affine as af
import _affine_phase as ap

CANVAS = ap.CANVAS


def test_shift_affine_is_the_warp_taken_at_another_origin():
    from offmark import resync
    f = np.array(ap.leak("svd", "B")[0])
    for g in (ap.geometry("B"), ap.geometry("B", -3.0, 1.1, (0.5, 0.25)), af.hflip(f.shape[1]), (0, af.ONE, 0, -af.ONE, 0, 90 << 16)):
        for py, px in ((0, 0), (1, 2), (7, 7), (3, 0), (0, 5), (13, 21)):
            s = resync.shift_affine(g, py, px)
            assert isinstance(s, tuple) and all(isinstance(v, int) for v in s) and s[:2] == tuple(g[:2]) and s[3:5] == tuple(g[3:5])
            got, inside = af.warp(f, s, CANVAS)
            ref, ref_inside = af.warp(f, g, CANVAS, origin=(py, px))
            assert np.array_equal(got, ref) and np.array_equal(inside, ref_inside)
        assert resync.shift_affine(g, 0, 0) == tuple(int(v) for v in g)
        assert resync.shift_affine(resync.shift_affine(g, 1, 2), 8, 16) == resync.shift_affine(g, 9, 18)
    many = ap.candidates("B")
    got = resync.shift_affine(many, 5, 3)
    assert got.dtype == np.int64 and got.shape == many.shape
    assert all(tuple(got[k]) == resync.shift_affine(many[k], 5, 3) for k in range(len(many)))
    big = resync.shift_affine((1 << 20, 1 << 20, 1 << 48, 0, 1 << 20, 0), 7, 7)      # Python integers: nothing wraps
    assert big[2] == (1 << 48) + 14 * (1 << 20)
    with pytest.raises(ValueError):
        resync.shift_affine((1, 2, 3, 4), 0, 0)


def test_one_warp_read_at_64_origins_is_the_statement():
    """The searches below use tests/_affine_phase.py's one_warp_statement; it is the statement's 64 separate warps, integer for
    integer, also for a flip, a map without units under some shifts and one out of range under its last shifts."""
    f = np.array(ap.leak("svd", "B")[1])
    h, w = f.shape[:2]
    edge = (af.ONE, 0, (1 << 48) - 3 * af.ONE, 0, af.ONE, 0)                    # in range alone, out of range from py = 4 on
    assert not ap.in_range(edge) and ap.in_range(af.hflip(w))
    for g in (ap.geometry("B", shift=(0.5, 0.5)), af.hflip(w), (af.ONE, 0, -(2 << 16), 0, af.ONE, -(4 << 16)), edge):
        s, u = ap.statement(f, CANVAS, g)
        s1, u1 = ap.one_warp_statement(f, CANVAS, g)
        assert np.array_equal(s, s1) and np.array_equal(u, u1)
        assert (s > 0).any() == (u > 0).any() == (g is not edge) and ((s > 0) == (u > 0)).all()
    assert int(ap.statement(f, CANVAS, ap.geometry("B", shift=(0.5, 0.5)))[1][8 * 1 + 2]) == 73


def test_subpixel_shifts_and_the_candidate_lists():
    from offmark import resync
    assert resync.subpixel_shifts() == (0.0, 0.5) == resync.subpixel_shifts(2) and resync.subpixel_shifts(1) == (0.0,)
    assert resync.subpixel_shifts(4) == (0.0, 0.25, 0.5, 0.75)
    with pytest.raises(ValueError):
        resync.subpixel_shifts(0)
    sub = resync.subpixel_shifts(2)
    k = resync.rotation_candidates(CANVAS, ap.leak_hw("B"), [2.0, 1.75, 2.25], [1.0], sub, sub)
    b = ap.candidates("B")
    assert k.shape == b.shape == (12, 6) and {tuple(g) for g in k} == {tuple(g) for g in b} and tuple(b[0]) == tuple(k[3])
    assert ap.candidates("A").shape == (7, 6) and len({tuple(g) for g in ap.candidates("A")}) == 7


def test_best_shifted_geometry_on_made_up_scores():
    from offmark import resync
    cands = ap.candidates("A")[:3]
    units = np.zeros((3, 64), np.int64)
    scores = np.zeros((2, 3, 64), np.int64)
    units[0, 10], units[0, 11], units[1, 5], units[2, 7] = 10, 20, 10, 0
    scores[:, 0, 10], scores[:, 0, 11], scores[:, 1, 5], scores[:, 2, 7] = 16384 * 8, 16384 * 10, 16384 * 4, 99
    b = resync.best_shifted_geometry(scores, units, cands)
    assert b["index"] == 0 and b["phase"] == (1, 2) and b["geometry"] == resync.shift_affine(cands[0], 1, 2)
    assert b["normalised"].shape == (3, 64) and b["normalised"][0, 10] == 0.8 and b["normalised"][0, 11] == 0.5 and b["normalised"][2, 7] == 0
    assert b["contrast"] == 2.0 and b["phase_contrast"] == 1.6
    assert resync.best_shifted_geometry(scores[0], units, cands)["normalised"][1, 5] == 0.4          # [K, 64]: one frame
    alone = resync.best_shifted_geometry(scores[:, 1:2], units[1:2], cands[1:2])
    assert alone["index"] == 0 and alone["phase"] == (0, 5) and alone["contrast"] == alone["phase_contrast"] == float("inf")
    with pytest.raises(ValueError):
        resync.best_shifted_geometry(scores, np.zeros((3, 64), np.int64), cands)


@pytest.mark.parametrize("which", ["A", "A2", "B"])
def test_the_truth_is_found_and_the_copies_are_read(which):
    from offmark import resync
    cands = ap.candidates(which)
    dec = ap.StatementDecoder()
    out = ap.read(dec, ap.leak("svd", which), cands)
    n = out["normalised"]
    k, p = out["index"], 8 * out["phase"][0] + out["phase"][1]
    print(f"leak {which}: index {k} phase {out['phase']} normalised {n[k, p]:.4f} contrast {out['contrast']:.4f} phase contrast "
          f"{out['phase_contrast']:.4f} best of the other candidates {np.delete(n, 0, axis=0).max():.4f} picks {[int(v) for v in out['picks']]} "
          f"base {out['base']} score {out['score']} runner-up {out['runner_up_score']}")
    assert list(out["picks"]) == list(af.CHOSEN) == [1, 0, 1] and not out["ambiguous"]
    assert out["index"] == 0
    if which != "A2":                                                          # A2 is another crop: its phase is its own
        assert out["phase"] == ap.TRUE_PHASE
    assert out["geometry"] == resync.shift_affine(cands[0], *out["phase"])
    assert out["contrast"] > 1.0 and out["phase_contrast"] > 1.0 and out["score"] > out["runner_up_score"]
    # on the unmarked sources attacked the same way, the best entry of the whole list stays below the marked truth's
    s, u = dec.affine_phase_scores_u8(ap.leak("none", which)[:ap.SEARCH_FRAMES], CANVAS, cands)
    un = resync.best_shifted_geometry(s, u, cands)["normalised"]
    print(f"leak {which} unmarked: best over the list {un.max():.4f}")
    assert un.max() < n[k, p]


def test_whole_pixel_shifts_alone_do_not_read_leak_b():
    """The documented reason for the sub-lattice: with the three angles at sub-pixel shift (0, 0) only, leak B's best entry is at
    the unmarked level and the copies read are not the marked ones."""
    cands = ap.whole_pixel_candidates("B")
    out = ap.read(ap.StatementDecoder(), ap.leak("svd", "B"), cands)
    print(f"leak B, whole pixels only: index {out['index']} phase {out['phase']} normalised {out['normalised'].max():.4f} picks "
          f"{[int(v) for v in out['picks']]}")
    assert list(out["picks"]) != [1, 0, 1]


def test_a_decoder_without_the_search_is_refused():
    import _warp as wp
    with pytest.raises(ValueError, match="affine"):                            # decode_soft_warp_u8 only, as DctDecoder
        ap.read(wp.StatementDecoder("dct"), ap.leak("svd", "A"), ap.candidates("A"))
    with pytest.raises(ValueError):
        ap.read(ap.StatementDecoder(), ap.leak("svd", "A"), wp.candidate_geometries()[:2])          # four columns: no linear part
