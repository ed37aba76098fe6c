"""CPU-only: a leaked clip's frames matched to the source video (offmark.temporal; build extensions) over the NumPy statements of
tests/_temporal.py, on its recipe: a 48-frame dissolve, the leak frames 11..40 with every sixth dropped, rotated and cropped (A) or
rotated and scaled (B).

Measured on the statement: the coarse map (8 x 8 thumbnails) is off by at most 1 frame on leak A and by 0 on leak B; register_leak
against those sources converges (luma rms 2.69 / 2.79); the residual path is exact for all 25 frames, after 2 rounds on A (the second
confirms) and 1 on B; the read-out returns segments [1, 2, 3, 4] with copies [0, 1, 1, 0]."""
import functools

import numpy as np
import pytest

import _align as al
import _temporal as tp

TRUTH = np.array(tp.KEPT)


@functools.lru_cache(maxsize=None)
def video_signatures():
    s = tp.signatures(tp.video())
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def coarse(which):
    from offmark import temporal
    return temporal.coarse_frame_map(tp.StatementDecoder(), tp.leak(which), video_signatures())


@functools.lru_cache(maxsize=None)
def read(which):
    from offmark import temporal
    return temporal.read_leak_clip(tp.StatementDecoder(), tp.leak(which), tp.video(), tp.PER, tp.CANVAS, tp.candidates(), key=tp.KEY, L=tp.L8,
                                   search_frames=tp.SEARCH_FRAMES, span=tp.SPAN, signatures=video_signatures())


# ---- the signature by hand ------------------------------------------------------------------------------------------------------
def test_a_signature_of_one_pixel_per_cell():
    frame = np.random.default_rng(1).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    want = [(int(p[0]) + 2 * int(p[1]) + int(p[2]) + 2) >> 2 for p in frame.reshape(64, 3)]
    assert tp.signature(frame).tolist() == want


def test_a_signature_of_uneven_cells():
    """13 rows split 1, 2, 1, 2, 2, 1, 2, 2 (edges (i * 13) >> 3) and 19 columns 2, 2, 3, 2, 2, 3, 2, 3."""
    frame = np.random.default_rng(2).integers(0, 256, (13, 19, 3), dtype=np.uint8)
    rows, cols = [0, 1, 3, 4, 6, 8, 9, 11, 13], [0, 2, 4, 7, 9, 11, 14, 16, 19]
    assert rows == [(i * 13) >> 3 for i in range(9)] and cols == [(j * 19) >> 3 for j in range(9)]
    want = []
    for i in range(8):
        for j in range(8):
            total, area = 0, 0
            for y in range(rows[i], rows[i + 1]):
                for x in range(cols[j], cols[j + 1]):
                    r, g, b = (int(v) for v in frame[y, x])
                    total += (r + 2 * g + b + 2) >> 2
                    area += 1
            want.append(int(np.floor(total / area + 0.5)))
    assert tp.signature(frame).tolist() == want


def test_a_mean_that_ends_in_a_half_rounds_up():
    frame = np.zeros((16, 16, 3), np.uint8)              # cells of 2 x 2 pixels
    frame[0, 0] = 2                                      # Y = 2: mean 0.5 -> 1
    frame[0, 2], frame[0, 3] = 5, 2                      # 7 / 4 = 1.75 -> 2
    frame[0, 4] = 1                                      # 0.25 -> 0
    frame[2, 0], frame[3, 1] = 255, 255                  # 127.5 -> 128
    frame[14:, 14:] = 255
    sig = tp.signature(frame)
    assert sig[:3].tolist() == [1, 2, 0] and sig[8] == 128 and sig[63] == 255 and int(sig.astype(int).sum()) == 1 + 2 + 128 + 255


def test_distances_by_hand():
    a = np.zeros((2, 64), np.uint8)
    b = np.full((3, 64), 255, np.uint8)
    b[1, :32] = 0
    b[2] = np.arange(64)
    a[1] = 63 - np.arange(64)
    want = [[16320, 8160, 2016], [16320 - 2016, (2016 - 496) + (8160 - 496), 2 * 32 * 32]]
    assert tp.distances(a, b).tolist() == want and tp.distances(a, b).dtype == np.int32


# ---- monotone_path by hand ------------------------------------------------------------------------------------------------------
INF = float("inf")


def path(cost, **kw):
    from offmark import temporal
    return temporal.monotone_path(np.asarray(cost, dtype=np.float64), **kw).tolist()


def test_a_path_with_a_dropped_and_a_doubled_frame():
    cost = np.full((5, 8), 9.0)
    for i, t in enumerate([2, 3, 5, 5, 6]):              # frame 4 dropped, frame 5 doubled
        cost[i, t] = 0.0
    assert path(cost) == [2, 3, 5, 5, 6]
    assert path(cost[:, ::-1]) != [5, 4, 2, 2, 1]        # a reversed clip is not followed


def test_the_max_step_bound():
    cost = np.full((2, 10), 5.0)
    cost[0, 1], cost[1, 8] = 0.0, 0.0                    # 7 frames apart
    assert path(cost, max_step=7) == [1, 8]
    assert path(cost, max_step=4) == [1, 1]              # total 5 either way: the smallest last frame, then the smallest step
    cost[1, 1] = 6.0
    assert path(cost, max_step=4) == [1, 2]
    assert path(cost, max_step=0) == [8, 8]              # 5 + 0 against 0 + 6 at frame 1


def test_a_masked_entry_is_not_taken():
    from offmark import temporal
    cost = np.array([[0.0, 1.0, 9.0], [9.0, 0.0, 1.0], [9.0, 9.0, 0.0]])
    assert path(cost) == [0, 1, 2]
    blocked = cost.copy()
    blocked[1, 1] = INF
    assert path(blocked) == [0, 2, 2]
    masked = np.ma.masked_array(cost, mask=np.zeros_like(cost, bool))
    masked[1, 1] = np.ma.masked
    assert temporal.monotone_path(masked).tolist() == [0, 2, 2]
    nan = cost.copy()
    nan[1, 1] = float("nan")
    assert path(nan) == [0, 2, 2]
    with pytest.raises(ValueError, match="no monotone path"):
        path([[INF, 0.0], [0.0, INF]])                   # only a step back would do
    with pytest.raises(ValueError):
        path(np.zeros(4))


def test_the_tie_rule():
    """Equal totals: the smallest last frame; walking back from it, the smallest step at every frame."""
    assert path(np.zeros((3, 5))) == [0, 0, 0]
    cost = np.array([[0.0, 0.0, 0.0, 9.0], [9.0, 9.0, 0.0, 0.0], [9.0, 9.0, 9.0, 0.0]])
    assert path(cost) == [2, 3, 3]                       # [0, 2, 3], [1, 2, 3], [2, 2, 3] and [1, 3, 3] cost the same
    ints = np.array([[3, 1, 1], [1, 1, 3]], dtype=np.int32)
    assert path(ints) == [1, 1]                          # totals 4, 2, 4 at the last frames 0, 1, 2; into frame 1 from 1, not from 0
    from offmark import temporal
    assert temporal.monotone_path(ints).dtype == np.int64


def test_torch_and_numpy_walk_the_same_path():
    import torch
    from offmark import temporal
    rng = np.random.default_rng(3)
    for m, N, step in ((1, 1, 4), (6, 5, 1), (25, 48, 4), (9, 30, 0), (12, 7, 127)):
        cost = rng.integers(0, 4, (m, N)).astype(np.float64)          # many ties
        cost[rng.random((m, N)) < 0.1] = INF
        cost[:, 0] = np.minimum(cost[:, 0], 3.0)                       # a path exists: stay at frame 0
        want = temporal.monotone_path(cost, step)
        got = temporal.monotone_path(torch.from_numpy(cost), step)
        assert isinstance(got, np.ndarray) and got.tolist() == want.tolist()
        assert (np.diff(want) >= 0).all() and (np.diff(want) <= step).all()
        # the minimum, against every path by dynamic programming written the other way round (forward sets)
        best = {t: cost[0, t] for t in range(N)}
        for i in range(1, m):
            best = {t: cost[i, t] + min(best[s] for s in range(max(0, t - step), t + 1)) for t in range(N)}
        assert cost[np.arange(m), want].sum() == min(best.values())


# ---- the recipe -----------------------------------------------------------------------------------------------------------------
def test_the_recipe_is_what_the_issue_says():
    assert tp.video().shape == (48, 72, 104, 3) and len(tp.KEPT) == 25 and tp.KEPT[0] == 11 and tp.KEPT[-1] == 39
    assert tp.leak("A").shape == (25, 56, 90, 3) and tp.leak("B").shape == (25, 72, 104, 3)
    assert sorted(set((TRUTH // tp.PER).tolist())) == tp.SEGMENTS and [1 - tp.CHOSEN[s] for s in tp.SEGMENTS] != tp.PICKS
    assert [tp.CHOSEN[s] for s in tp.SEGMENTS] == tp.PICKS


@pytest.mark.parametrize("which", tp.LEAKS)
def test_every_coarse_error_is_within_the_refinement_window(which):
    got = coarse(which)
    err = np.abs(got["frame_map"] - TRUTH)
    print(f"leak {which}: coarse errors {err.tolist()}; distance at the map {got['cost'].tolist()}")
    assert err.max() <= tp.SPAN // 2 == 3
    assert (np.diff(got["frame_map"]) >= 0).all() and (got["row_min"] <= got["cost"]).all() and (got["row_min"] <= got["row_second"]).all()
    assert got["frame_map"].dtype == np.int64 and got["cost"].shape == got["row_min"].shape == got["row_second"].shape == (25,)


@pytest.mark.parametrize("which", tp.LEAKS)
def test_the_refined_map_is_the_truth(which):
    from offmark import resync, temporal
    dec, leak, k = tp.StatementDecoder(), tp.leak(which), tp.SEARCH_FRAMES
    start = coarse(which)["frame_map"]
    report = resync.register_leak(dec, tp.video()[start[:k]], leak[:k], tp.CANVAS)
    assert report["converged"]
    got = temporal.refine_frame_map(dec, leak, tp.video(), tp.CANVAS, start, report["geometry"], span=tp.SPAN)
    assert got.tolist() == TRUTH.tolist() and got.dtype == np.int64
    # a library window that starts at frame 4: the same map in the video's numbering
    win = temporal.refine_frame_map(dec, leak, tp.video()[4:], tp.CANVAS, start, report["geometry"], library_start=4, span=tp.SPAN)
    assert win.tolist() == TRUTH.tolist()


@pytest.mark.parametrize("which", tp.LEAKS)
def test_a_clip_is_read_with_no_frame_map_given(which):
    got = read(which)
    print(f"leak {which}: rounds {got['rounds_used']} rms {got['registration']['rms']:.3f} residual max {got['residual'].max():.2f} "
          f"picks {[int(p) for p in got['picks']]}")
    assert got["frame_map"].tolist() == TRUTH.tolist() and got["coarse_frame_map"].tolist() == coarse(which)["frame_map"].tolist()
    assert got["segments"] == tp.SEGMENTS and [int(p) for p in got["picks"]] == tp.PICKS and not got["ambiguous"] and got["base"] == 0
    assert got["registration"]["converged"] and got["registration"]["rms"] < 4.0 and 1 <= got["rounds_used"] <= 2
    assert got["residual"].shape == (25,) and np.isfinite(got["residual"]).all()
    assert set(got) >= {"index", "phase", "geometry", "normalised", "contrast", "phase_contrast", "segments", "soft_by_segment", "base", "picks",
                        "score", "runner_up_score", "ambiguous", "registration", "frame_map", "coarse_frame_map", "rounds_used", "residual"}
    assert got["geometry"] == got["registration"]["geometry"] and got["runner_up_score"] is None


def test_without_the_frame_map_the_existing_read_out_fails():
    """The state before offmark.temporal, kept so the contrast stays visible: sources[i] = video[i] for a clip that starts at frame 11
    does not register, labels the segments 0..3 and returns other copies."""
    from offmark import resync
    leak = tp.leak("A")
    n = len(leak)
    cands = tp.candidates()
    got = resync.read_registered_leak(tp.StatementDecoder(), leak, tp.video()[:n], np.arange(n) // tp.PER, tp.CANVAS, cands, key=tp.KEY,
                                      L=tp.L8, search_frames=tp.SEARCH_FRAMES)
    print(f"converged {got['registration']['converged']} rms {got['registration']['rms']} segments {got['segments']} "
          f"picks {[int(p) for p in got['picks']]}")
    assert not got["registration"]["converged"]
    assert got["segments"] == [0, 1, 2, 3] and [int(p) for p in got["picks"]] != tp.PICKS


def test_the_library_window_and_the_decoder_are_checked():
    from offmark import temporal
    dec, cands = tp.StatementDecoder(), tp.candidates()
    kw = dict(key=tp.KEY, L=tp.L8, search_frames=tp.SEARCH_FRAMES, span=tp.SPAN)
    with pytest.raises(ValueError, match=r"needs source frames 4\.\.46, the library holds 5\.\.47"):
        temporal.read_leak_clip(dec, tp.leak("B"), tp.video()[5:], tp.PER, tp.CANVAS, cands, signatures=video_signatures(), library_start=5, **kw)
    with pytest.raises(ValueError, match=r"needs source frames 4\.\.46, the library holds 0\.\.45"):
        temporal.read_leak_clip(dec, tp.leak("B"), tp.video()[:46], tp.PER, tp.CANVAS, cands, signatures=video_signatures(), **kw)
    with pytest.raises(ValueError, match="library_start"):
        temporal.read_leak_clip(dec, tp.leak("B"), tp.video()[4:], tp.PER, tp.CANVAS, cands, library_start=4, **kw)
    with pytest.raises(ValueError, match="signatures_u8"):
        temporal.read_leak_clip(al.StatementDecoder(), tp.leak("B"), tp.video(), tp.PER, tp.CANVAS, cands, **kw)
    # the window 4..46 is enough, in the video's numbering; and the signatures default to the library's
    got = temporal.read_leak_clip(dec, tp.leak("B"), tp.video()[4:47], tp.PER, tp.CANVAS, cands, signatures=video_signatures(), library_start=4, **kw)
    assert got["frame_map"].tolist() == TRUTH.tolist() and [int(p) for p in got["picks"]] == tp.PICKS
    own = temporal.read_leak_clip(dec, tp.leak("B"), tp.video(), tp.PER, tp.CANVAS, cands, **kw)
    assert own["frame_map"].tolist() == TRUTH.tolist() and own["geometry"] == read("B")["geometry"]


def test_the_residual_statement_is_the_alignment_sums():
    """Entries [27] and [28] of tests/_align.py's sums for the gathered pair; (0, 0) outside the library."""
    lib, leak, geom = tp.video()[:3], tp.leak("B")[:2], read("B")["geometry"]
    got = tp.residuals(lib, leak, [-1, 1], 3, geom)
    assert got.shape == (2, 3, 2) and not got[0, 0].any() and not got[1, 2].any()
    assert got[0, 1].tolist() == al.sums(lib[0], leak[0], geom)[27:29].tolist() and got[1, 1].tolist() == al.sums(lib[2], leak[1], geom)[27:29].tolist()
    assert got[0, 1, 1] > 4000
