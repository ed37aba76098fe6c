"""CPU-only: a leaked clip whose tone changed, matched to the source video and read (offmark.temporal.read_toned_leak_clip; build
extensions) over the NumPy statements of tests/_toned_clip.py: tests/_temporal.py's recipe (a 48-frame dissolve; the leak is frames
11..40 with every sixth dropped, rotated and cropped (A) or rotated and scaled (B)) sent through tests/_tone.py's five tone maps and
through the identity, 12 cases.

Measured with this file, on the statement:
  coarse    the path through the RANK distances is within 3 frames (A) and 2 frames (B) of the truth -- marginal at span // 2 = 3;
            after the signature refits (3 in every case) within 2 frames (A, 15-17 of 25 exact) and 1 frame (B, 25 of 25 exact in five
            cases, 23 under gamma 1.20);
  exact     the correlation path is the truth for 25 of 25 frames in all 12 cases, after 2 rounds on A (the second confirms), 1 on B
            (2 under gamma 1.20); the cost at the map has median 0.013-0.015 and maximum 0.11;
  read      segments [1, 2, 3, 4], copies [0, 1, 1, 0], not ambiguous, converged, luma rms 2.69 (A) and 2.79 (B);
  before    read_leak_clip on the ten toned clips leaves the library (both gamma 0.85 and both combined cases) or returns other
            copies from a map with 1-19 of 25 frames exact; sum e^2 on the tone-fitted leak A stays at 23 of 25 under every map."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import _align as al
import _temporal as tp
import _tone as tn
import _toned_clip as tc

TRUTH = np.array(tp.KEPT)
CASES = [(which, name) for which in tp.LEAKS for name in tc.MAPS]
KW = dict(key=tp.KEY, L=tp.L8, search_frames=tp.SEARCH_FRAMES, span=tp.SPAN)


@functools.lru_cache(maxsize=None)
def coarse(which, name):
    from offmark import temporal
    return temporal.coarse_frame_map_toned(tc.StatementDecoder(), tc.toned(which, name), tc.video_signatures())


@functools.lru_cache(maxsize=None)
def read(which, name):
    from offmark import temporal
    return temporal.read_toned_leak_clip(tc.StatementDecoder(), tc.toned(which, name), tp.video(), tp.PER, tp.CANVAS, tp.candidates(),
                                         signatures=tc.video_signatures(), **KW)


# ---- the two statements ---------------------------------------------------------------------------------------------------------
def test_the_moments_give_the_residual_and_its_count():
    """[3] + [4] - 2 [5] and [0] are tests/_align.py's sums [27] and [28] of the pair; six zeros outside the library."""
    lib, leak = tp.video()[9:14], tc.toned("A", "gamma-0.85")[:2]
    for geom in (tc.af.IDENTITY, (65000, 2300, 5 << 16, -2300, 65000, 3 << 16)):
        got = tc.moments(lib, leak, [-1, 3], 3, geom)
        assert got.shape == (2, 3, 6) and got.dtype == np.int64 and not got[0, 0].any() and not got[1, 2].any()
        for i, j, s in ((0, 1, 0), (0, 2, 1), (1, 0, 3), (1, 1, 4)):
            sse, cnt = al.sums(lib[s], leak[i], geom)[27:29]
            assert got[i, j, 3] + got[i, j, 4] - 2 * got[i, j, 5] == sse and got[i, j, 0] == cnt > 4000
        assert (got[0, 1:, :2] == got[0, 1, :2]).all() and (got[0, 1:, 3] == got[0, 1, 3]).all()      # n, sum l, sum l^2: the leak's alone
    assert not tc.moments(lib, leak, [0, 0], 2, (0,) * 6).any()                                     # a geometry out of range


def test_a_moment_by_hand():
    """An 8 x 8 canvas under the identity: the 6 x 6 interior of a 8 x 8 leak."""
    rng = np.random.default_rng(5)
    lib, leak = rng.integers(0, 256, (1, 8, 8, 3), dtype=np.uint8), rng.integers(0, 256, (1, 8, 8, 3), dtype=np.uint8)
    n = sl = ss = sll = sss = sls = 0
    for y in range(1, 7):
        for x in range(1, 7):
            l = (int(leak[0, y, x, 0]) + 2 * int(leak[0, y, x, 1]) + int(leak[0, y, x, 2]) + 2) >> 2
            s = (int(lib[0, y, x, 0]) + 2 * int(lib[0, y, x, 1]) + int(lib[0, y, x, 2]) + 2) >> 2
            n, sl, ss, sll, sss, sls = n + 1, sl + l, ss + s, sll + l * l, sss + s * s, sls + l * s
    assert tc.moments(lib, leak, [0], 1, tc.af.IDENTITY)[0, 0].tolist() == [n, sl, ss, sll, sss, sls] and n == 36


def test_ranks_are_a_permutation_with_ties_broken_by_the_index():
    flat = np.full((1, 64), 77, np.uint8)
    assert tc.ranks(flat)[0].tolist() == list(range(64))                                             # all equal: the identity
    down = (200 - 3 * np.arange(64)).astype(np.uint8)[None]
    assert tc.ranks(down)[0].tolist() == list(range(63, -1, -1))                                     # strictly decreasing
    tied = np.random.default_rng(11).integers(0, 6, (5, 64)).astype(np.uint8)                        # six values over 64 cells
    got = tc.ranks(tied)
    assert got.dtype == np.uint8 and got.shape == (5, 64)
    for f in range(5):
        assert sorted(got[f].tolist()) == list(range(64))
        assert got[f].tolist() == np.argsort(np.argsort(tied[f], kind="stable"), kind="stable").tolist()
        order = np.argsort(got[f])
        assert (np.diff(tied[f][order].astype(int)) >= 0).all()
        same = np.diff(tied[f][order].astype(int)) == 0
        assert (np.diff(order)[same] > 0).all()                                                      # equal values: the index decides
    sig = tc.video_signatures()[:4]
    for name in tn.TONE_MAPS:                                                                        # an increasing curve keeps the order
        a, b, gamma = tn.TONE_MAPS[name]
        strict = a * np.arange(256.0) + b
        strict = strict if gamma == 1.0 else 255.0 * (np.clip(strict, 1e-9, None) / 255.0) ** gamma
        assert (np.diff(strict) > 0).all()
        assert np.array_equal(tc.ranks(sig), np.argsort(np.argsort(strict[sig], axis=1, kind="stable"), axis=1, kind="stable"))


# ---- the host side by hand ------------------------------------------------------------------------------------------------------
def moments_of(l, s):
    l, s = [int(v) for v in l], [int(v) for v in s]
    return [len(l), sum(l), sum(s), sum(v * v for v in l), sum(v * v for v in s), sum(a * b for a, b in zip(l, s))]


def test_ncc_cost_does_not_see_a_gain_or_an_offset_and_masks_a_flat_side():
    from offmark import temporal
    rng = np.random.default_rng(7)
    l, s = rng.integers(0, 256, 500), rng.integers(0, 256, 500)
    s = (s + 2 * l) // 3                                                     # correlated
    base = moments_of(l, s)
    n, sl, ss, sll, sss, sls = base
    a, b, c = n * sll - sl * sl, n * sss - ss * ss, n * sls - sl * ss
    exact = Fraction(c * abs(c), a * b)
    assert 0 < exact < 1
    cost = temporal.ncc_cost(np.asarray([base], np.int64), 384)
    assert cost.shape == (1,) and cost[0] == 1.0 - (c * abs(c)) / (a * b) and abs(cost[0] - float(1 - exact)) < 1e-15
    for g, o in ((3, 0), (1, 40), (7, -900), (2, 11)):                       # l -> g l + o: the rational is the same, so is the float
        n2, sl2, ss2, sll2, sss2, sls2 = m2 = moments_of(g * l + o, s)
        a2, c2 = n2 * sll2 - sl2 * sl2, n2 * sls2 - sl2 * ss2
        assert Fraction(c2 * abs(c2), a2 * b) == exact
        assert temporal.ncc_cost(np.asarray([m2], np.int64), 384)[0] == cost[0]
        m3 = moments_of(l, g * s + o)                                        # and on the source's side
        assert temporal.ncc_cost(np.asarray([m3], np.int64), 384)[0] == cost[0]
    assert temporal.ncc_cost(np.asarray([moments_of(255 - l, s)], np.int64), 384)[0] == 2.0 - cost[0] > 1      # a negative gain is no match
    assert temporal.ncc_cost(np.asarray([moments_of(s, s)], np.int64), 384)[0] == 0.0
    flat = np.full(500, 9)
    masked = temporal.ncc_cost(np.asarray([[moments_of(flat, s), moments_of(l, flat)], [base, [0] * 6]], np.int64), 384)
    assert masked.shape == (2, 2) and np.isinf(masked[0]).all() and masked[1, 0] == cost[0] and np.isinf(masked[1, 1])
    assert np.isinf(temporal.ncc_cost(np.asarray([base], np.int64), 501)[0])                                   # too few pixels
    big = [1 << 24, 255 << 23, 255 << 23, (255 * 255) << 23, (255 * 255) << 23, 0]                             # products beyond int64
    assert temporal.ncc_cost(np.asarray([big], np.int64), 384)[0] == 2.0                                       # half 0, half 255, opposed
    with pytest.raises(ValueError):
        temporal.ncc_cost(np.zeros((2, 5), np.int64), 384)
    with pytest.raises(ValueError):
        temporal.ncc_cost(np.zeros((2, 6)), 384)


def test_signature_lut_recovers_a_known_curve():
    from offmark import temporal, tone
    sig = tc.video_signatures()[10:35]
    x = np.arange(256, dtype=np.float64)
    known = np.clip(np.rint(0.7 * x + 40), 0, 255).astype(np.uint8)
    lut = temporal.signature_lut(sig, known[sig])
    have = np.unique(sig)
    assert lut.dtype == np.uint8 and lut.shape == (256,) and (np.diff(lut.astype(int)) >= 0).all()
    assert np.array_equal(lut[have], known[have]) and have.size > 100
    table = np.zeros((3, 256, 2), np.int64)                                   # tone.lut_of_sums' rules, by its own code
    np.add.at(table[0, :, 0], sig.reshape(-1), 1)
    np.add.at(table[0, :, 1], sig.reshape(-1), known[sig].reshape(-1).astype(np.int64))
    assert np.array_equal(tone.lut_of_sums(table)[0], lut)
    one = np.full((2, 64), 5, np.uint8)
    assert np.array_equal(temporal.signature_lut(one, one), np.arange(256))    # fewer than 2 leak values: the identity
    with pytest.raises(ValueError):
        temporal.signature_lut(sig, known[sig][:, :32])


# ---- the grid: both leaks x (the five tone maps + the identity) -----------------------------------------------------------------
@pytest.mark.parametrize("which,name", CASES)
def test_the_coarse_map_is_within_the_refinement_window(which, name):
    got = coarse(which, name)
    rank_err, err = np.abs(got["rank_frame_map"] - TRUTH), np.abs(got["frame_map"] - TRUTH)
    print(f"leak {which} {name}: rank path errors max {rank_err.max()} exact {(rank_err == 0).sum()}; after {got['refits_used']} refits max "
          f"{err.max()} exact {(err == 0).sum()}")
    assert rank_err.max() <= 3 and err.max() <= 2
    assert 1 <= got["refits_used"] <= 3 and (np.diff(got["frame_map"]) >= 0).all() and got["frame_map"].dtype == np.int64
    assert (got["row_min"] <= got["cost"]).all() and got["cost"].shape == got["row_min"].shape == got["row_second"].shape == (25,)


@pytest.mark.parametrize("which,name", CASES)
def test_a_toned_clip_is_read_with_no_frame_map_given(which, name):
    got = read(which, name)
    print(f"leak {which} {name}: rounds {got['rounds_used']} rms {got['registration']['rms']:.3f} ncc median {np.median(got['ncc']):.4f} max "
          f"{got['ncc'].max():.4f} picks {[int(p) for p in got['picks']]}")
    assert got["frame_map"].tolist() == TRUTH.tolist() and got["coarse_frame_map"].tolist() == coarse(which, name)["frame_map"].tolist()
    assert got["segments"] == tp.SEGMENTS and [int(p) for p in got["picks"]] == tp.PICKS and not got["ambiguous"]
    assert got["registration"]["converged"] and 1 <= got["rounds_used"] <= 2
    assert got["ncc"].shape == (25,) and np.isfinite(got["ncc"]).all() and (got["ncc"] >= 0).all()
    assert set(got) >= {"geometry", "segments", "picks", "score", "ambiguous", "registration", "tone", "frame_map", "coarse_frame_map",
                        "rounds_used", "ncc"}
    assert got["tone"]["lut"].shape == (3, 256) and (np.diff(got["tone"]["lut"].astype(int), axis=1) >= 0).all()


def test_the_refits_use_no_more_than_asked_and_none_gives_the_rank_path():
    from offmark import temporal
    dec, leak = tc.StatementDecoder(), tc.toned("A", "gamma-0.85")
    none = temporal.coarse_frame_map_toned(dec, leak, tc.video_signatures(), refits=0)
    assert none["refits_used"] == 0 and none["frame_map"].tolist() == none["rank_frame_map"].tolist() == coarse("A", "gamma-0.85")["rank_frame_map"].tolist()
    one = temporal.coarse_frame_map_toned(dec, leak, tc.video_signatures(), refits=1)
    assert one["refits_used"] == 1
    ranks = tc.ranks(tc.video_signatures())
    assert none["cost"].tolist() == tp.distances(tc.ranks(tp.signatures(leak)), ranks)[np.arange(25), none["frame_map"]].tolist()


# ---- kept on record: what the project did with such clips before -------------------------------------------------------------------
@pytest.mark.parametrize("which", tp.LEAKS)
@pytest.mark.parametrize("name", list(tn.TONE_MAPS))
def test_the_plain_clip_read_out_leaves_the_library_or_returns_other_copies(which, name):
    from offmark import temporal
    try:
        got = temporal.read_leak_clip(tc.StatementDecoder(), tc.toned(which, name), tp.video(), tp.PER, tp.CANVAS, tp.candidates(),
                                      signatures=tc.video_signatures(), **KW)
    except ValueError as e:
        print(f"leak {which} {name}: {e}")
        assert "needs source frames" in str(e)
        return
    exact = int((got["frame_map"] == TRUTH).sum())
    print(f"leak {which} {name}: {exact} of 25 frames exact, picks {[int(p) for p in got['picks']]}")
    assert exact < 25 and [int(p) for p in got["picks"]] != tp.PICKS


@pytest.mark.parametrize("name", ["gamma-0.85", "gain-0.70+40-gamma-1.10"])
def test_the_residual_on_the_tone_fitted_leak_falls_short_where_the_correlation_does_not(name):
    """Leak A: histogram match, registration and the tone_sums curve on the coarse map's nearly-right sources; the curve absorbs the
    brightness error of a frame that is one off, so sum e^2 of the fitted leak keeps 2 frames wrong.  The correlation of the RAW leak
    at the same geometry is exact."""
    from offmark import resync, temporal, tone
    dec, leak, k = tc.StatementDecoder(), tc.toned("A", name), tp.SEARCH_FRAMES
    start = coarse("A", name)["frame_map"]
    src = tp.video()[start[:k]]
    lut0 = tone.lut_of_histograms(tn.histograms(leak[:k]).sum(axis=0), tn.histograms(src).sum(axis=0))
    report = resync.register_leak(dec, src, tn.apply_tone(leak[:k], lut0), tp.CANVAS)
    lut = tone.lut_of_sums(tn.statement_sums(src, leak[:k], [report["geometry"]]).sum(axis=0)[0])
    by_residual = temporal.refine_frame_map(dec, tn.apply_tone(leak, lut), tp.video(), tp.CANVAS, start, report["geometry"], span=tp.SPAN)
    by_ncc = temporal.refine_frame_map_ncc(dec, leak, tp.video(), tp.CANVAS, start, report["geometry"], span=tp.SPAN)
    print(f"leak A {name}: residual {(by_residual == TRUTH).sum()} of 25, correlation {(by_ncc == TRUTH).sum()} of 25")
    assert report["converged"] and (by_residual == TRUTH).sum() < 25
    assert by_ncc.tolist() == TRUTH.tolist() and by_ncc.dtype == np.int64
    win = temporal.refine_frame_map_ncc(dec, leak, tp.video()[4:], tp.CANVAS, start, report["geometry"], library_start=4, span=tp.SPAN)
    assert win.tolist() == TRUTH.tolist()


# ---- the arguments --------------------------------------------------------------------------------------------------------------
def test_the_library_window_and_the_decoder_are_checked():
    from offmark import temporal
    dec, cands, leak = tc.StatementDecoder(), tp.candidates(), tc.toned("B", "gain-0.85+15")
    sig = tc.video_signatures()
    with pytest.raises(ValueError, match=r"needs source frames 4\.\.46, the library holds 5\.\.47"):
        temporal.read_toned_leak_clip(dec, leak, tp.video()[5:], tp.PER, tp.CANVAS, cands, signatures=sig, library_start=5, **KW)
    with pytest.raises(ValueError, match=r"needs source frames 4\.\.46, the library holds 0\.\.45"):
        temporal.read_toned_leak_clip(dec, leak, tp.video()[:46], tp.PER, tp.CANVAS, cands, signatures=sig, **KW)
    with pytest.raises(ValueError, match="library_start"):
        temporal.read_toned_leak_clip(dec, leak, tp.video()[4:], tp.PER, tp.CANVAS, cands, library_start=4, **KW)
    with pytest.raises(ValueError, match="signatures_u8"):
        temporal.read_toned_leak_clip(al.StatementDecoder(), leak, tp.video(), tp.PER, tp.CANVAS, cands, **KW)
    with pytest.raises(ValueError, match="signature_ranks_u8"):                    # the plain clip's decoder lacks the two new calls
        temporal.read_toned_leak_clip(tp.StatementDecoder(), leak, tp.video(), tp.PER, tp.CANVAS, cands, **KW)
    with pytest.raises(ValueError, match="rounds"):
        temporal.read_toned_leak_clip(dec, leak, tp.video(), tp.PER, tp.CANVAS, cands, rounds=0, **KW)
    with pytest.raises(ValueError, match="dict"):
        temporal.read_toned_leak_clip(dec, leak, tp.video(), tp.PER, tp.CANVAS, [cands], **KW)
    # the window 4..46 is enough, in the video's numbering; and the signatures default to the library's
    got = temporal.read_toned_leak_clip(dec, leak, tp.video()[4:47], tp.PER, tp.CANVAS, cands, signatures=sig, library_start=4, **KW)
    assert got["frame_map"].tolist() == TRUTH.tolist() and [int(p) for p in got["picks"]] == tp.PICKS
    own = temporal.read_toned_leak_clip(dec, leak, tp.video(), tp.PER, tp.CANVAS, cands, **KW)
    assert own["frame_map"].tolist() == TRUTH.tolist() and own["geometry"] == read("B", "gain-0.85+15")["geometry"] == got["geometry"]
