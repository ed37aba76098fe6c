"""Reading a leaked CLIP: which source frame each leak frame came from (build extension, not reference semantics).

Every read-out in offmark.resync takes the time axis as known: ``read_registered_leak`` needs ``sources[i]`` to be frame i's source.  A
real leak starts somewhere in the video, a frame-rate conversion has dropped (or doubled) frames, and it is rotated, rescaled and cropped
on top.  With sources[i] = video[i] the registration of such a leak does not converge and the copies it returns are wrong
(tests/test_temporal_statement.py keeps that case).  The map leak frame -> source frame is found in two passes, both over integer
statements (include/offmark_hip.h; tests/_temporal.py), so the device and NumPy routes agree exactly:

  coarse   an 8 x 8 luma thumbnail per frame (decoder.signatures_u8) and the L1 distances between the leak's and the video's
           (decoder.signature_distances_u8); a monotone path through that matrix (``monotone_path``) puts every leak frame within
           +-1 of its source on the test recipe, although the leak is rotated and cropped: the thumbnail is coarse enough.
  exact    ``register_leak`` against those nearly-right sources converges, and the luma residual at the registered geometry
           (decoder.align_residuals_u8: sum e^2 and the pixel count of every leak frame against ``span`` sources around its current
           one) is sharply minimal at the true frame -- on the recipe 1.2 against 81-83 one frame off, and still 6.1 against 78-93
           when the registration itself used sources one frame off.  A second monotone path through the residuals is the exact map.

``read_leak_clip`` runs both, registers once more on the exact map and hands over to the existing read-out.

A re-graded or screen-captured clip changes its brightness, contrast or gamma as well, and both passes above lose their footing: in a
dissolve brightness IS time, so the plain thumbnail's strongest cue moves, and sum e^2 sees a gain before it sees a wrong frame.
``read_toned_leak_clip`` makes both passes tone invariant (tests/_toned_clip.py) and hands over to offmark.tone.read_toned_leak:

  coarse   the path through the distances between RANK signatures (decoder.signature_ranks_u8: a cell's place among the 64, which no
           increasing curve changes), then up to three refits: the monotone curve leak signature byte -> library signature byte at the
           current path (``signature_lut``), the PLAIN distances of the mapped signatures, the path again (``coarse_frame_map_toned``);
  exact    registration on the histogram-matched leak, then the zero-mean normalised cross-correlation of the RAW leak's warped luma
           with each of ``span`` sources, from six integer sums (decoder.align_moments_u8, ``ncc_cost``): a gain and an offset cancel
           exactly, a gamma nearly (``refine_frame_map_ncc``).  The residual of a tone-FITTED leak is not enough: a curve fitted on
           nearly-right sources absorbs the brightness error of a frame that is one off.

What neither can do: clips re-cut out of order or reversed (the path is monotone); a tone curve that varies over the clip or over the
frame, or cross-talk between channels (for a leak whose frames are already matched, offmark.colour.read_coloured_leak fits the colour
matrix; for a clip it is not built); static content, where time is not observable, and pure pans, where a time shift and a crop offset
are the same thing; the DCT codec, 4:2:0 planes, blk 8."""
from __future__ import annotations

import numpy as np

from . import resync, tone

MAX_SPAN = 16                 # sources per leak frame of one decoder.align_residuals_u8 call


def _is_tensor(x) -> bool:
    return hasattr(x, "is_cuda") and hasattr(x, "data_ptr")


def monotone_path(cost, max_step: int = 4) -> np.ndarray:
    """The cheapest monotone path through a cost matrix.  cost: [m, N], NumPy or torch; +inf, NaN or a masked entry (numpy.ma) means
    "not allowed".  -> int64 [m], the t_0..t_{m-1} with 0 <= t_i - t_{i-1} <= max_step that minimise sum_i cost[i][t_i]; any t_0.
    Step 0 is a doubled frame, a step above 1 dropped frames; there is no step penalty.  Raises ValueError when no path is allowed.
    Tie rule: among paths of equal total the one with the smallest last frame t_{m-1}, and, walking back from it, at every frame the
    smallest step (the latest predecessor).  Sums are float64: integer costs below 2^53 / m are exact and ties between them too.
    On torch the m sequential N-wide steps, the int8 back-pointers and the walk back stay on the tensor's device; only the path comes to
    the host."""
    max_step = int(max_step)
    if not 0 <= max_step <= 127:
        raise ValueError("max_step must be in 0..127 (the back-pointers are int8)")
    if _is_tensor(cost):
        import torch
        xp, c = torch, cost.to(torch.float64)
        c = torch.where(torch.isnan(c), torch.full_like(c, float("inf")), c)
        full = lambda n, v, dt: torch.full((n,), v, dtype=dt, device=c.device)
        cat, i8, i64 = torch.cat, torch.int8, torch.int64
    else:
        xp = np
        c = np.ma.filled(np.ma.asarray(cost, dtype=np.float64), np.inf) if np.ma.isMaskedArray(cost) else np.asarray(cost, dtype=np.float64)
        c = np.where(np.isnan(c), np.inf, c)
        full = lambda n, v, dt: np.full((n,), v, dtype=dt)
        cat, i8, i64 = np.concatenate, np.int8, np.int64
    if c.ndim != 2 or c.shape[0] < 1 or c.shape[1] < 1:
        raise ValueError("cost must be [m, N] with m, N >= 1")
    m, N = int(c.shape[0]), int(c.shape[1])
    total = c[0]
    back = []
    for i in range(1, m):
        best, step = total, full(N, 0, i8)
        for s in range(1, min(max_step, N - 1) + 1):
            cand = cat((full(s, float("inf"), c.dtype), total[:N - s]))  # cand[t] = total[t - s]
            better = cand < best                                       # strictly: the smaller step stays on a tie
            best = xp.where(better, cand, best)
            step = xp.where(better, full(N, s, i8), step)
        back.append(step)
        total = c[i] + best
    low = total.min()
    if not bool(low < float("inf")):
        raise ValueError("no monotone path is allowed through this cost matrix")
    if xp is np:
        t = int(np.flatnonzero(total == low)[0])
        path = np.empty(m, np.int64)
        for i in range(m - 1, -1, -1):
            path[i] = t
            if i:
                t -= int(back[i - 1][t])
        return path
    t = (total == low).nonzero()[0, 0].reshape(1)
    path = xp.empty(m, dtype=i64, device=c.device)
    for i in range(m - 1, -1, -1):
        path[i:i + 1] = t
        if i:
            t = t - back[i - 1].gather(0, t).to(i64)
    return path.cpu().numpy()


def _needs(decoder, names, what) -> None:
    for need in names:
        if not hasattr(decoder, need):
            raise ValueError(f"{type(decoder).__name__} does not {what} ({need}): only DwtDctSvd does")


def coarse_frame_map(decoder, frames, signatures, max_step: int = 4) -> dict:
    """The leak's frames placed in the video by their thumbnails.  decoder: anything with DwtDctSvdDecoder's signatures_u8 /
    signature_distances_u8; frames: uint8 [m, h, w, 3], the leak; signatures: uint8 [N, 64], the signatures of the WHOLE video, index 0 =
    frame 0 (where ``frames`` lives: a device tensor for a device decoder; a host array is copied there).  -> dict(frame_map int64 [m]
    (monotone_path of the distances), cost int64 [m] (the distance at the map), row_min, row_second int64 [m] (the smallest and the second
    smallest distance of each leak frame over the whole video; equal when the video has one frame): how well the thumbnails tell the
    frames apart)."""
    _needs(decoder, ("signatures_u8", "signature_distances_u8"), "compute frame signatures")
    mine = decoder.signatures_u8(frames)
    return _placed(decoder.signature_distances_u8(mine, _beside(mine, signatures)), max_step)


def _beside(mine, other):
    """``other`` (uint8) where ``mine`` lives: on its device when it is a tensor and ``other`` is a host array."""
    if _is_tensor(mine) and not _is_tensor(other):
        import torch
        return torch.from_numpy(np.ascontiguousarray(np.asarray(other, dtype=np.uint8))).to(mine.device)
    return other


def _placed(dist, max_step) -> dict:
    """coarse_frame_map's dict of a distance matrix [m, N]."""
    path = monotone_path(dist, max_step)
    d = resync._host(dist).astype(np.int64)
    two = np.sort(d, axis=1)[:, :2]
    return dict(frame_map=path, cost=d[np.arange(d.shape[0]), path], row_min=two[:, 0].copy(), row_second=two[:, -1].copy())


def signature_lut(leak_sigs, matched_sigs) -> np.ndarray:
    """The monotone curve leak signature byte -> library signature byte of a matched pair of signature lists, both uint8 [m, 64] on the
    host: the table [256][2] = (count, sum of the library's bytes) per leak byte goes through offmark.tone.curve_of_sums (isotonic fit,
    interpolation, one rounding).  -> uint8 [256], non-decreasing; the identity when fewer than 2 leak values occur."""
    a, b = np.asarray(leak_sigs), np.asarray(matched_sigs)
    if a.shape != b.shape or a.ndim != 2 or a.shape[1] != 64 or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError("both signature lists must be uint8 [m, 64]")
    table = np.zeros((tone.LEVELS, 2), np.int64)
    np.add.at(table[:, 0], a.reshape(-1), 1)
    np.add.at(table[:, 1], a.reshape(-1), b.reshape(-1).astype(np.int64))
    return tone.curve_of_sums(table)


def coarse_frame_map_toned(decoder, frames, signatures, max_step: int = 4, refits: int = 3) -> dict:
    """coarse_frame_map for a leak whose tone changed.  In a dissolve brightness IS time, so the plain thumbnail's strongest cue is what
    a tone change destroys.  decoder: anything with DwtDctSvdDecoder's signatures_u8 / signature_ranks_u8 / signature_distances_u8; the
    other arguments are coarse_frame_map's.
      1. the path through the distances between the RANK signatures of the leak and of the video (decoder.signature_ranks_u8: invariant
         under any increasing tone curve, but blind to a frame's overall level);
      2. at most ``refits`` times: signature_lut of the leak's signatures against the video's at the current path, the PLAIN distances of
         the leak's signatures mapped through it, the path again; stop when the path repeats.
    -> coarse_frame_map's keys (of the last distances; the rank distances' when refits = 0) plus rank_frame_map int64 [m] and
    refits_used."""
    _needs(decoder, ("signatures_u8", "signature_ranks_u8", "signature_distances_u8"), "compute tone-invariant frame signatures")
    mine = decoder.signatures_u8(frames)
    signatures = _beside(mine, signatures)
    out = _placed(decoder.signature_distances_u8(decoder.signature_ranks_u8(mine), decoder.signature_ranks_u8(signatures)), max_step)
    rank_map, used = out["frame_map"], 0
    mine_host, video_host = np.asarray(resync._host(mine)), np.asarray(resync._host(signatures))
    for _ in range(int(refits)):
        before = out["frame_map"]
        lut = signature_lut(mine_host, video_host[before])
        out = _placed(decoder.signature_distances_u8(_beside(mine, np.ascontiguousarray(lut[mine_host])), signatures), max_step)
        used += 1
        if np.array_equal(out["frame_map"], before):
            break
    out.update(rank_frame_map=rank_map, refits_used=used)
    return out


def _mse_cost(res, min_pixels) -> np.ndarray:
    """align_residuals_u8's (sum e^2, count) [m, span, 2] -> sum e^2 / count, float64 [m, span]; +inf below ``min_pixels`` pixels."""
    sse, cnt = res[..., 0], res[..., 1]
    return np.where(cnt >= int(min_pixels), sse / np.maximum(cnt, 1), np.inf)


def ncc_cost(moments, min_pixels: int = 384) -> np.ndarray:
    """decoder.align_moments_u8's sums -> 1 - the signed square of the zero-mean normalised cross-correlation of the leak's warped luma l
    and a source's luma s.  moments: integers [..., 6] = (n, sum l, sum s, sum l^2, sum s^2, sum l s).  In Python integers
    a = n sum l^2 - (sum l)^2, b = n sum s^2 - (sum s)^2, c = n sum l s - sum l sum s; the entry is c |c| / (a b) away from 1, ONE
    correctly rounded division, so the same integers give the same float64 wherever they were formed; +inf (masked) where n <
    ``min_pixels`` or either side is flat (a <= 0 or b <= 0).  -> float64 [...], 0 (l = g s + o, g > 0) .. 2 (g < 0).  A gain and an
    offset on either side cancel exactly, and a gamma nearly does."""
    mom = np.asarray(resync._host(moments))
    if mom.ndim < 1 or mom.shape[-1] != 6 or mom.dtype.kind not in "iu":
        raise ValueError("moments must be integers [..., 6]")
    flat = mom.reshape(-1, 6).tolist()                                  # Python integers: the products leave int64
    out = np.full(len(flat), np.inf)
    for k, (n, sl, ss, sll, sss, sls) in enumerate(flat):
        a, b, c = n * sll - sl * sl, n * sss - ss * ss, n * sls - sl * ss
        if n >= int(min_pixels) and a > 0 and b > 0:
            out[k] = 1.0 - (c * abs(c)) / (a * b)
    return out.reshape(mom.shape[:-1])


def _refine(decoder, frames, library, canvas_hw, frame_map, geom, library_start, span, min_pixels, max_step, sums="align_residuals_u8",
            cost_of=_mse_cost):
    """One decoder call (``sums``: align_residuals_u8 or align_moments_u8) over the windows first = frame_map - span // 2 -
    library_start, ``cost_of`` on what it returns, monotone_path through the costs -> (the new map, the cost at it)."""
    fm = np.asarray(frame_map, dtype=np.int64).reshape(-1)
    span = int(span)
    if not 1 <= span <= MAX_SPAN:
        raise ValueError(f"span must be in 1..{MAX_SPAN}")
    if fm.size != int(frames.shape[0]):
        raise ValueError("frame_map needs one entry per leak frame")
    first = fm - span // 2 - int(library_start)                         # indices into ``library``
    res = resync._host(getattr(decoder, sums)(library, frames, canvas_hw, first.astype(np.int32), span, geom)).astype(np.int64)
    window = cost_of(res, min_pixels)                                   # [m, span]; a source outside the library has count 0: +inf
    lo = int(first.min())
    cost = np.full((fm.size, int(first.max()) - lo + span), np.inf)
    for i in range(fm.size):
        cost[i, first[i] - lo:first[i] - lo + span] = window[i]
    path = monotone_path(cost, max_step)
    return path + lo + int(library_start), cost[np.arange(fm.size), path]


def refine_frame_map(decoder, frames, library, canvas_hw, frame_map, geom, library_start: int = 0, span: int = 7, min_pixels: int = 384,
                     max_step: int = 4) -> np.ndarray:
    """A nearly-right frame map made exact from the luma residual at a registered geometry.  library: uint8 [N, H, W, 3], source frames
    ``library_start``..; frame_map: [m] source-frame numbers (of the whole video), each within span // 2 of the truth; geom: the leak's
    affine geometry (register_leak).  One decoder.align_residuals_u8 call with first = frame_map - span // 2 - library_start; the cost
    of leak frame i at a source is sum e^2 / count, masked where fewer than ``min_pixels`` pixels contribute (register_leak's floor) or
    the source lies outside the library; monotone_path through it -> the new map, int64 [m]."""
    return _refine(decoder, frames, library, canvas_hw, frame_map, geom, library_start, span, min_pixels, max_step)[0]


def refine_frame_map_ncc(decoder, frames, library, canvas_hw, frame_map, geom, library_start: int = 0, span: int = 7, min_pixels: int = 384,
                         max_step: int = 4) -> np.ndarray:
    """refine_frame_map for a leak whose tone changed: decoder.align_moments_u8 and ncc_cost in place of sum e^2 / count.  ``frames``
    is the RAW leak: the correlation does not see a gain or an offset, while a tone curve fitted on nearly-right sources absorbs the
    brightness error of a frame that is one off and takes the residual's minimum with it."""
    return _refine(decoder, frames, library, canvas_hw, frame_map, geom, library_start, span, min_pixels, max_step, "align_moments_u8",
                   ncc_cost)[0]


def _take(frames, index):
    if _is_tensor(frames):
        import torch
        return frames.index_select(0, torch.from_numpy(np.ascontiguousarray(index, dtype=np.int64)).to(frames.device))
    return np.ascontiguousarray(np.asarray(frames)[index])


def _clip_arguments(decoder, library, frames_per_segment, candidates, rounds, signatures, library_start):
    """The argument checks the clip read-outs share -> (frames per segment, library_start, rounds, the whole video's signatures)."""
    _needs(decoder, ("align_sums_u8", "halve_u8", "decode_soft_affine_u8"), "read at an affine geometry")
    per, start, rounds = int(frames_per_segment), int(library_start), int(rounds)
    if per < 1 or rounds < 1 or start < 0:
        raise ValueError("frames_per_segment and rounds must be at least 1, library_start at least 0")
    if not isinstance(candidates, dict):
        raise ValueError("candidates must be a dict keyed by absolute segment number")
    if signatures is None:
        if start != 0:
            raise ValueError("without signatures of the whole video the library must start at frame 0 (library_start = 0)")
        signatures = decoder.signatures_u8(library)
    return per, start, rounds, signatures


def _library_holds(fmap, span, start, library) -> None:
    """Each round may move a frame by span // 2 and reads span // 2 beyond: the coarse map -+ span must lie inside the library."""
    need = (int(fmap.min()) - int(span), int(fmap.max()) + int(span))
    have = (start, start + int(library.shape[0]) - 1)
    if need[0] < have[0] or need[1] > have[1]:
        raise ValueError(f"the clip needs source frames {need[0]}..{need[1]}, the library holds {have[0]}..{have[1]}")


def read_leak_clip(decoder, frames, library, frames_per_segment: int, canvas_hw, candidates, key=0, L: int = 8, search_frames: int = 8,
                   span: int = 7, rounds: int = 2, signatures=None, library_start: int = 0, max_step: int = 4, **register) -> dict:
    """A leaked clip's copy per segment, read against the source video with NO frame map given.  decoder: a DwtDctSvdDecoder (blk 4;
    anything with its signatures_u8 / signature_distances_u8 / align_residuals_u8 / align_sums_u8 / halve_u8 / decode_soft_affine_u8 --
    a DctDecoder raises ValueError); frames: uint8 [m, h, w, 3], the leak in playing order; library: uint8 [N, H, W, 3], the source
    frames ``library_start``.. of the video (unmarked or marked); frames_per_segment: source frames per segment, segment s being frames
    s * frames_per_segment ..; candidates: a dict keyed by ABSOLUTE segment number -> the payloads that segment may carry; signatures:
    uint8 [frames of the whole video, 64], index 0 = frame 0 -- when None they are computed from ``library``, and library_start must
    then be 0; ``register``: start, levels, max_iters, tol_px of register_leak.
      1. coarse_frame_map;
      2. at most ``rounds`` times: register_leak on the first ``search_frames`` leak frames against library[map - library_start],
         refine_frame_map over all frames at that geometry; stop when the map no longer changes;
      3. a final register_leak on the exact map (the last one is kept where the map did not change after it);
      4. all frames are read at that geometry (decoder.decode_soft_affine_u8);
      5. segment_of_frame = frame_map // frames_per_segment, align_segments with bases (0,).
    Raises ValueError, naming the source frames it needs, when the coarse map -+ span leaves the library (each round may move a frame by
    span // 2 and reads span // 2 beyond).  -> read_registered_leak's keys plus frame_map, coarse_frame_map (int64 [m]), rounds_used and
    residual (float [m]: sum e^2 / count of every frame at the final map, under the geometry of the last refinement).  No verdict: judge
    ``registration['converged']`` and the residuals."""
    canvas_hw = (int(canvas_hw[0]), int(canvas_hw[1]))
    _needs(decoder, ("signatures_u8", "signature_distances_u8", "align_residuals_u8"), "match a clip's frames to its source")
    per, start, rounds, signatures = _clip_arguments(decoder, library, frames_per_segment, candidates, rounds, signatures, library_start)
    coarse = coarse_frame_map(decoder, frames, signatures, max_step)
    fmap = coarse["frame_map"]
    _library_holds(fmap, span, start, library)
    k = max(1, int(search_frames))
    report, rounds_used, settled, residual = None, 0, False, None
    for _ in range(rounds):
        report = resync.register_leak(decoder, _take(library, fmap[:k] - start), frames[:k], canvas_hw, **register)
        nxt, residual = _refine(decoder, frames, library, canvas_hw, fmap, report["geometry"], start, span, resync.ALIGN_MIN_PIXELS, max_step)
        rounds_used += 1
        settled = bool(np.array_equal(nxt, fmap))
        fmap = nxt
        if settled:
            break
    if not settled:
        report = resync.register_leak(decoder, _take(library, fmap[:k] - start), frames[:k], canvas_hw, **register)
    geom = report["geometry"]
    normalised = None
    if hasattr(decoder, "affine_scores_u8") and report["units"] > 0:
        s = resync._host(decoder.affine_scores_u8(frames[:k], canvas_hw, np.asarray([geom], dtype=np.int64))).astype(np.int64)
        normalised = float(s.sum()) / (float(resync.ONE) * report["units"] * s.shape[0])
    soft = decoder.decode_soft_affine_u8(frames, canvas_hw, geom, L)
    out = resync._align_by_segment(soft, fmap // per, candidates, key, bases=(0,))
    out.update(index=0, phase=(0, 0), geometry=geom, normalised=normalised, contrast=None, phase_contrast=None, registration=report,
               frame_map=fmap, coarse_frame_map=coarse["frame_map"], rounds_used=rounds_used, residual=residual)
    return out


def read_toned_leak_clip(decoder, frames, library, frames_per_segment: int, canvas_hw, candidates, key=0, L: int = 8, search_frames: int = 8,
                         span: int = 7, rounds: int = 2, signatures=None, library_start: int = 0, max_step: int = 4, **register) -> dict:
    """read_leak_clip for a clip whose brightness, contrast or gamma changed as well (a re-grade, a screen capture); the arguments are
    read_leak_clip's.  decoder: a DwtDctSvdDecoder (blk 4; anything with its signature_ranks_u8 / align_moments_u8 on top of what
    read_leak_clip and offmark.tone.read_toned_leak need -- a DctDecoder raises ValueError).  With k = ``search_frames``:
      1. coarse_frame_map_toned;
      2. at most ``rounds`` times: tone.lut_of_histograms of the first k leak frames against library[map[:k] - library_start],
         register_leak on the leak mapped through that table, refine_frame_map_ncc of the RAW leak over all frames at that geometry;
         stop when the map no longer changes;
      3. tone.read_toned_leak on library[map - library_start] with segment_of_frame = map // frames_per_segment: it fits the curve,
         registers again and reads.
    Raises read_leak_clip's ValueErrors.  -> read_toned_leak's dict plus frame_map, coarse_frame_map (int64 [m]), rounds_used and ncc
    (float [m]: ncc_cost of every frame at the final map, under the geometry of the last refinement).  No verdict: judge
    ``registration['converged']``, its ``rms`` and ``ncc``."""
    canvas_hw = (int(canvas_hw[0]), int(canvas_hw[1]))
    _needs(decoder, ("signatures_u8", "signature_ranks_u8", "signature_distances_u8", "align_moments_u8"),
           "match a toned clip's frames to its source")
    _needs(decoder, ("histograms_u8", "tone_sums_u8", "apply_tone_u8"), "fit a tone curve")
    per, start, rounds, signatures = _clip_arguments(decoder, library, frames_per_segment, candidates, rounds, signatures, library_start)
    coarse = coarse_frame_map_toned(decoder, frames, signatures, max_step)
    fmap = coarse["frame_map"]
    _library_holds(fmap, span, start, library)
    k = max(1, int(search_frames))
    leak_hist = tone._frame_sum(decoder.histograms_u8(frames[:k]))
    rounds_used, ncc = 0, None
    for _ in range(rounds):
        sources = _take(library, fmap[:k] - start)
        lut0 = tone.lut_of_histograms(leak_hist, tone._frame_sum(decoder.histograms_u8(sources)))
        report = resync.register_leak(decoder, sources, decoder.apply_tone_u8(frames[:k], lut0), canvas_hw, **register)
        nxt, ncc = _refine(decoder, frames, library, canvas_hw, fmap, report["geometry"], start, span, resync.ALIGN_MIN_PIXELS, max_step,
                           "align_moments_u8", ncc_cost)
        rounds_used += 1
        settled = bool(np.array_equal(nxt, fmap))
        fmap = nxt
        if settled:
            break
    out = tone.read_toned_leak(decoder, frames, _take(library, fmap - start), fmap // per, canvas_hw, candidates, key=key, L=L,
                               search_frames=search_frames, **register)
    out.update(frame_map=fmap, coarse_frame_map=coarse["frame_map"], rounds_used=rounds_used, ncc=ncc)
    return out
