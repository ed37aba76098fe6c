"""Reading CROPPED leaks: block-grid resync for the DwtDctSvd and the DCT read-out (host side, NumPy only).

Build extension, not reference semantics.  A crop does two mechanical things to a block-transform mark:
  * it moves the PHASE of the 8x8 unit grid (64 possibilities), and
  * it changes the frame's block count, so the position rule (unit index mod L) scrambles the payload positions.
DwtDctSvd (blk 4) has no frame-global dependency: a unit's read-out depends on its own 8x8 pixels only.  At the right phase a
cropped leak's units are therefore exactly the marked frame's units, and both effects can be undone:
  1. ``DwtDctSvdDecoder.sync_scores_u8`` gives, per phase, the sum of |soft metric| over the phase's units; on the marked grid
     every unit sits at +-2^14, on any other grid (and on unmarked content) the mean is near 0.7 * 2^14: ``best_phase``.
  2. ``DwtDctSvdDecoder.decode_soft_window_u8`` reads the units of that phase with the positions of the UNCROPPED frame's width
     (``canvas_cols``); what is then unknown is one rotation of the L positions -- the crop's whole units above and left of the
     leak -- common to every frame of the leak: ``align_segments`` resolves it against the publisher's own candidate payloads.
The DCT codec HAS a frame-global dependency, the luminance mask's frame mean.  ``DctDecoder`` has the same two methods: its masks
and frame mean come from the leak as received -- per phase, from the contiguous crop that holds the phase's full blocks, as the
decoder treats any received frame -- so the right phase reads near, not at, +-2^14 per block (the leak's mean is not the marked
frame's, and the marking itself moved the masks).  On the oracle-marked test recipe (3 segments x 4 frames of 72x104, alpha 20,
cropped to 61x83) the right phase scores 0.991 normalised against a median of 0.786 over the other phases; ``best_phase``'s
contrast is 1.183 there (1.187 on a second seed set, 1.197 on 136x200 cropped at (19, 37), 1.163 on 40x56 cropped at (5, 3)) and
1.005 on the unmarked sources cropped the same way.  That is lower than DwtDctSvd's 1.28-1.45: C21 is a low-frequency coefficient
and neighbouring phases correlate -- a property of the codec.  ``best_phase``, ``align_segments`` and ``units_per_phase`` are the
same for both codecs.
``read_cropped_leak`` is the recipe end to end, with either decoder.
4:2:0 PLANES (I420 / NV12) are read at EVEN crop offsets, without an RGB intermediate: ``read_cropped_leak_yuv420`` over the
decoders' ``sync_scores_planes_yuv420`` / ``decode_soft_window_planes_yuv420`` and ``best_phase(..., even_only=True)``.  A crop at
even pixel offsets cuts sub-planes out of the marked planes, and the build-defined conversion replicates chroma over its 2x2
cell, so converting the cropped planes gives the crop of the converted frame byte for byte: on the test recipe marked through
planes -> RGB -> oracle encoder -> planes and cropped at (10, 20) or (2, 6), both codecs return the right phase, base and copies,
with contrast 1.30-1.33 (DwtDctSvd) and 1.106-1.115 (DCT) over the 16 even phases, against 1.003-1.012 on the unmarked sources.
A crop at an ODD offset cannot exist on 4:2:0 planes without resampling chroma by half a sample, and that destroys a mark that
lives in U: made through RGB (convert, crop at (11, 21), convert back) the same leak reads with contrast 1.017 / 1.005, wrong
phase and wrong copies.  That is a property of a chroma mark under 4:2:0, not of the search, so on planes the 48 phases with an
odd py or px score 0 and take no part.
RESCALED leaks (cropped and zoomed back, or re-encoded at another resolution; interleaved RGB) have lost the 8x8 grid.  They are
resampled back onto the marked frame's pixel grid (the canvas) with the inverse of the crop and scale -- an integer bilinear warp,
``warp_of_crop`` -- and the canvas units that fall wholly inside the leak (``warp_units``) are read with the same unit metric, at
the positions they have in the uncropped frame: no rotation is left.  ``DwtDctSvdDecoder.warp_scores_u8`` scores a list of
candidate geometries (``crop_candidates``) in one fused call, ``best_geometry`` ranks them, ``decode_soft_warp_u8`` (both decoders)
reads at one geometry: ``read_rescaled_leak``.  The score is as sharp as the phase search -- one crop edge off by a pixel falls to
the unmarked level, rows and columns do not separate -- and only DwtDctSvd has a search: the DCT codec's C21 is small on smooth
resampled content whether marked or not, so it reads at a geometry known from the sizes or found by other means.
ROTATED leaks (and sheared, flipped or turned ones; interleaved RGB, DwtDctSvd only) are the same recipe under a 2x3 integer
affine map: ``affine_of_rotation`` / ``affine_of_warp`` make one, ``affine_units`` gives the counting units (convex, no longer a
rectangle), ``rotation_candidates`` a list, and ``best_geometry`` / ``read_rescaled_leak`` take [K, 6] lists as well as [K, 4]
(``DwtDctSvdDecoder.affine_scores_u8`` / ``decode_soft_affine_u8``).  The parameters have to be right all at once: an angle off by
0.25 degrees already falls to the unmarked level.  The DCT codec has no affine read-out: its frame mean and masks would have to
come from a non-rectangular set of blocks.
ROTATED-AND-CROPPED leaks (rotated or rescaled, then cropped off-centre: the normal case) have an unknown translation, and that
is the one part of a geometry that needs no list.  A shift of the canvas by whole pixels (py, px) is an exact integer change of
the map's offsets, ``shift_affine``: by' = by + ayy * py + ayx * px, bx' = bx + axy * py + axx * px.  The shifts by 0..7 px are
the 64 phases of the unit grid on the warped canvas -- ``DwtDctSvdDecoder.affine_phase_scores_u8`` scores all 64 of every
candidate in one call, ``best_shifted_geometry`` ranks the K x 64 entries -- and shifts by whole units only rotate the payload
positions, which ``align_segments`` resolves as for cropped leaks: ``read_transformed_leak``.  What still has to be listed is the
LINEAR part (angle, scale) and the SUB-PIXEL shift (``subpixel_shifts``).  Measured on the NumPy statement (tests/_affine_phase.py:
the 72x104 recipe rotated by 2 degrees and cropped, first 4 frames):
  * rows 7:63 / columns 5:95: the truth scores 0.740 normalised at phase (1, 2) on 65 units, its second phase 0.677, angles off by
    0.25 / 0.5 degrees and scale +-1 % at most 0.706 over all phases, the unmarked sources at most 0.699; copies [1, 0, 1] with
    an alignment score of 7.85 M against 4.46 M for the runner-up base;
  * rows 7:64 / columns 5:96 (odd sizes move the index centre by half a pixel): whole-pixel shifts alone reach 0.691, the
    unmarked level, and return wrong copies; with the sub-pixel shift (0.5, 0.5) the truth scores 0.742 on 73 units against at
    most 0.695 elsewhere and the copies come out (9.28 M against 5.04 M).  Hence the 2 x 2 half-pixel sub-lattice;
  * the fall-off: the score's peak is about a quarter of a pixel wide -- 0.754 at the exact translation, about 0.70 at 0.06 to
    0.125 px, the unmarked level from 0.19 px on, and at 0.25 to 0.5 px the best of all 64 phases is 0.67-0.69 -- and a
    quarter-pixel lattice gains nothing on the recipe.  The half-pixel lattice is enough for whole-pixel crops of a frame rotated
    about its centre (the translation is then within about 0.1 px of a multiple of half a pixel); it is NOT a cover of an
    arbitrary translation, which takes subpixel_shifts(8).
The contrasts are thin (about 1.05 between candidates, 1.07-1.09 between phases on 4 small frames): no verdict is given.
WITH THE SOURCE FRAMES AT HAND -- the operator who reads a leak marked the video -- nothing has to be listed: ``register_leak`` fits
the leak's geometry to its source, six parameters by Gauss-Newton on the luma difference between the warped leak and the source,
coarse to fine over a pyramid of 2x2 halvings (``level_down`` / ``level_up`` carry a geometry between levels), each step
(``align_step``) from 29 integer sums per frame that ``DwtDctSvdDecoder.align_sums_u8`` computes in one fused call without writing a
warped frame.  The result lies on the source's own pixel grid, so ``read_registered_leak`` reads with base 0 and no search.  On the
NumPy statement (tests/_align.py, the leaks above, first 4 frames, from the centred UNROTATED start) the registered geometry lies
0.10 / 0.08 px at the canvas corners from the listed truth of the two leaks and reads a stronger mark than it (sum |m| per unit
12.9 k / 12.6 k against 12.1 k / 12.2 k; 10.0 k / 10.2 k for the unmarked sources registered the same way); a leak rotated by -3
degrees with step 1.10 registers from scale 1 to 0.016 px; starts shifted by (12, 10) and (-16, 14) px need one halving.
4:2:0 planes under any resampling, blk 8, perspective, the DCT codec under an affine map and, without the source frames, a search
of the linear part itself (anything beyond scoring a given list of linear parts and sub-pixel shifts) are not handled.
"""
from __future__ import annotations

import numpy as np

ONE = 16384      # the soft metric's fixed point (2^14)


def units_per_phase(H: int, W: int) -> np.ndarray:
    """int64 [64]: full 8x8 units of an H x W frame at phase (py, px), at index 8 * py + px; 0 where none fits."""
    r = np.maximum((H - np.arange(8)) // 8, 0).astype(np.int64)
    c = np.maximum((W - np.arange(8)) // 8, 0).astype(np.int64)
    return (r[:, None] * c[None, :]).reshape(64)


def _rank(s: np.ndarray, units: np.ndarray, have: np.ndarray) -> tuple:
    """The ranking behind best_phase and best_geometry.  s: int64 [n, K] scores (rows are added); units: int64 [K] units behind
    each entry; have: bool [K], the entries that take part (at least one) -> (normalised float64 [K], 0 where not ``have``; the
    best entry's index, the first on a tie; contrast = best / second best, inf when there is no second or it scores 0)."""
    norm = np.zeros(units.size, np.float64)
    norm[have] = s.sum(axis=0)[have] / (float(ONE) * units[have] * s.shape[0])
    order = np.argsort(-np.where(have, norm, -1.0), kind="stable")
    top = int(order[0])
    second = float(norm[order[1]]) if have.sum() > 1 else 0.0
    return norm, top, float(norm[top] / second) if second > 0 else float("inf")


def best_phase(scores, H: int, W: int, even_only: bool = False) -> dict:
    """scores: [64] or [n, 64] sums of |soft metric| per phase (rows are added) of H x W frames ->
    dict(phase=(py, px), normalised=float64 [64], contrast=top / second).  normalised = score / (2^14 * units * frames): about 1
    on the marked grid; phases without units are excluded (0 there).  No verdict: the caller judges ``contrast``, which is about
    1.0 on flat content (a flat frame carries no phase information) and inf when one phase at most has units or the
    second-best scores 0.  ``even_only`` (4:2:0 planes): only the phases with even py and px take part -- in the ranking, in
    ``contrast`` and in ``normalised`` (0 elsewhere)."""
    s = np.asarray(scores, dtype=np.int64).reshape(-1, 64)
    units = units_per_phase(H, W)
    have = units > 0
    if even_only:
        even = np.arange(8) % 2 == 0
        have &= (even[:, None] & even[None, :]).reshape(64)
    if not have.any():
        raise ValueError(f"a {H}x{W} frame holds no 8x8 unit")
    norm, top, contrast = _rank(s, units, have)
    return dict(phase=(top // 8, top % 8), normalised=norm, contrast=contrast)


def shuffled(payload, key) -> np.ndarray:
    """The payload as the marked frames carry it at positions 0..L-1: Shuffler(key)'s permutation."""
    from .generator.shuffler import Shuffler
    p = np.asarray(payload).reshape(-1)
    return np.asarray(Shuffler(key=key).generate_wm(p, (p.size,))).reshape(-1)


def align_segments(soft_by_segment, candidates, key, bases=None) -> dict:
    """One rotation of the L payload positions, common to all segments, and per segment the candidate it then reads as.
    soft_by_segment: [S, L] soft sums read with base 0; candidates[s]: the payloads (L bits each) segment s may carry.
    With T[s][q] = soft[s][(q - base) % L], maximises over base in 0..L-1
        sum_s max_k sum_q (2 * shuffled(candidates[s][k])[q] - 1) * T[s][q]
    (integers, so ties are exact).  -> dict(base, picks int [S] (index into candidates[s]; the first on a tie), score,
    runner_up_score (the best other base's), ambiguous (another base, or another candidate of a segment at the best base, scores
    the same)).  ``bases``: the rotations that take part (default: all L); (0,) for sums read in canvas coordinates, where no
    rotation is left -- runner_up_score is then None."""
    soft = np.asarray(soft_by_segment, dtype=np.int64)
    if soft.ndim != 2 or len(candidates) != soft.shape[0]:
        raise ValueError("soft_by_segment must be [S, L] with one candidate list per segment")
    S, L = soft.shape
    signs = []
    for s in range(S):
        c = np.stack([2 * shuffled(p, key).astype(np.int64) - 1 for p in candidates[s]])
        if c.shape[1] != L:
            raise ValueError(f"candidates of segment {s} are not {L} bits long")
        signs.append(c)
    bases = list(range(L)) if bases is None else [int(b) % L for b in bases]
    if not bases:
        raise ValueError("bases must name at least one rotation")
    totals = np.empty(len(bases), np.int64)
    picks = np.empty((len(bases), S), np.int64)
    tied_pick = np.zeros(len(bases), bool)
    for b, base in enumerate(bases):
        T = np.roll(soft, base, axis=1)                    # T[s][q] = soft[s][(q - base) % L]
        total = 0
        for s in range(S):
            corr = signs[s] @ T[s]
            k = int(np.argmax(corr))
            picks[b, s] = k
            tied_pick[b] |= int((corr == corr[k]).sum()) > 1
            total += int(corr[k])
        totals[b] = total
    best = int(np.argmax(totals))
    others = np.delete(totals, best)
    runner_up = int(others.max()) if others.size else None
    ambiguous = bool(tied_pick[best] or (runner_up is not None and runner_up == int(totals[best])))
    return dict(base=bases[best], picks=picks[best].copy(), score=int(totals[best]), runner_up_score=runner_up, ambiguous=ambiguous)


def _host(x) -> np.ndarray:
    return np.asarray(x.cpu() if hasattr(x, "cpu") else x)


def _align_by_segment(soft, segment_of_frame, candidates, key, bases=None) -> dict:
    """The tail of the read_*_leak recipes.  soft: [n, L] soft sums per frame; segment_of_frame: [n] labels -> align_segments of
    the sums per segment (candidates in the order of the sorted distinct labels, or a dict keyed by label), with ``segments``
    (the sorted labels) and ``soft_by_segment`` added."""
    soft = _host(soft).astype(np.int64)
    seg = np.asarray(segment_of_frame).reshape(-1)
    if seg.size != soft.shape[0]:
        raise ValueError("segment_of_frame needs one entry per frame")
    labels = sorted(set(seg.tolist()))
    by_segment = np.stack([soft[seg == s].sum(axis=0) for s in labels])
    cands = [candidates[s] for s in labels] if isinstance(candidates, dict) else list(candidates)
    out = align_segments(by_segment, cands, key, bases)
    out.update(segments=labels, soft_by_segment=by_segment)
    return out


def read_cropped_leak(decoder, frames, segment_of_frame, canvas_width: int, candidates, key=0, L: int = 8, search_frames: int = 8) -> dict:
    """A cropped leak's copy per segment.  decoder: a DwtDctSvdDecoder (blk 4) or a DctDecoder (anything with their
    sync_scores_u8 / decode_soft_window_u8); frames: CUDA uint8 [n, H, W, 3], the leak as it is
    (any H, W >= 8); segment_of_frame: [n] segment label per frame; canvas_width: the marked (uncropped) frames' width in pixels;
    candidates: per segment, in the order of the sorted distinct labels (or a dict keyed by label), the payloads it may carry.
    Phase search on the first ``search_frames`` frames, window read-out of all frames at the best phase with base 0, sums per
    segment, align_segments.  -> dict(phase, contrast, normalised, segments (the sorted labels), soft_by_segment, base, picks,
    score, runner_up_score, ambiguous).  No verdict on ``contrast``: about 1.0 means the frames carried no phase information.
    With a DctDecoder the masks and the frame mean come from the leak as received, so the right phase reads near, not at, +-2^14
    per block and ``contrast`` is lower than DwtDctSvd's: 1.18 on the marked test recipe against 1.005 on its unmarked sources
    (module docstring)."""
    H, W = int(frames.shape[1]), int(frames.shape[2])
    found = best_phase(_host(decoder.sync_scores_u8(frames[:max(1, int(search_frames))])), H, W)
    soft = decoder.decode_soft_window_u8(frames, L, found["phase"], int(canvas_width) // 8, base=0)
    out = _align_by_segment(soft, segment_of_frame, candidates, key)
    out.update(phase=found["phase"], contrast=found["contrast"], normalised=found["normalised"])
    return out


def read_cropped_leak_yuv420(decoder, planes, height: int, width: int, segment_of_frame, canvas_width: int, candidates, key=0, L: int = 8,
                             search_frames: int = 8, layout: str = "i420") -> dict:
    """read_cropped_leak for a leak that arrives as 4:2:0 planes, cropped at EVEN pixel offsets (module docstring: an odd offset
    cannot exist on planes).  decoder: a DwtDctSvdDecoder (blk 4) or a DctDecoder (anything with their sync_scores_planes_yuv420 /
    decode_soft_window_planes_yuv420); planes: CUDA uint8 [n, 1.5 * height * width] in ``layout`` ("i420" / "nv12"), height and
    width even and >= 8; the other arguments and the returned dict as read_cropped_leak.  The phase search ranks the 16 even
    phases only (best_phase(..., even_only=True)); nothing is converted to RGB."""
    H, W = int(height), int(width)
    found = best_phase(_host(decoder.sync_scores_planes_yuv420(planes[:max(1, int(search_frames))], H, W, layout=layout)), H, W, even_only=True)
    soft = decoder.decode_soft_window_planes_yuv420(planes, H, W, L, found["phase"], int(canvas_width) // 8, base=0, layout=layout)
    out = _align_by_segment(soft, segment_of_frame, candidates, key)
    out.update(phase=found["phase"], contrast=found["contrast"], normalised=found["normalised"])
    return out


# ---- rescaled leaks: the warp onto the marked frame's canvas ------------------------------------------------------------------
WARP_ONE = 1 << 16                     # the warp's fixed point (Q16)
WARP_MIN_A, WARP_MAX_A = 1 << 12, 1 << 20


def _round_div(num: int, den: int) -> int:
    """round(num / den), halves up, in exact integers (den > 0)."""
    return (2 * num + den) // (2 * den)


def warp_of_crop(top: int, left: int, ch: int, cw: int, h: int, w: int) -> tuple:
    """(ay, by, ax, bx), Q16: the map canvas pixel -> sample of a leak of h x w pixels that was made from canvas rows
    top:top+ch and columns left:left+cw with half-pixel centres.  ay = round(h/ch * 2^16),
    by = round(((0.5 - top) * h/ch - 0.5) * 2^16), columns alike; exact integer rounding, halves up."""
    top, left, ch, cw, h, w = (int(v) for v in (top, left, ch, cw, h, w))
    if ch < 1 or cw < 1 or h < 1 or w < 1:
        raise ValueError("crop and leak sizes must be positive")
    ay, ax = _round_div(h * WARP_ONE, ch), _round_div(w * WARP_ONE, cw)
    by = _round_div(((1 - 2 * top) * h - ch) * (WARP_ONE // 2), ch)
    bx = _round_div(((1 - 2 * left) * w - cw) * (WARP_ONE // 2), cw)
    return ay, by, ax, bx


def _axis_units(a: int, b: int, length: int, units: int) -> tuple:
    u = np.arange(units, dtype=np.int64)
    ok = (a * (8 * u) + b >= 0) & (((a * (8 * u + 7) + b) >> 16) <= length - 1)
    idx = np.flatnonzero(ok)
    return (int(idx[0]), int(idx[-1]) + 1) if idx.size else (0, 0)


def warp_units(leak_hw, canvas_hw, geom) -> tuple:
    """(i0, i1, j0, j1): the canvas units (i < H // 8, j < W // 8) whose 64 pixels all fall inside the leak under ``geom``
    (0 <= pos >> 16 <= size - 1 on both axes); the maps are monotone, so they form a rectangle.  All 0 when none counts.
    Equal to the library's ofmk_warp_units."""
    ay, by, ax, bx = (int(v) for v in np.asarray(geom).reshape(-1))
    if not (WARP_MIN_A <= ay <= WARP_MAX_A and WARP_MIN_A <= ax <= WARP_MAX_A):
        raise ValueError("ay and ax must be in [2^12, 2^20]")
    i0, i1 = _axis_units(ay, by, int(leak_hw[0]), int(canvas_hw[0]) // 8)
    j0, j1 = _axis_units(ax, bx, int(leak_hw[1]), int(canvas_hw[1]) // 8)
    return (i0, i1, j0, j1) if i1 > i0 and j1 > j0 else (0, 0, 0, 0)


def crop_candidates(canvas_hw, leak_hw, tops, lefts, heights, widths) -> np.ndarray:
    """int64 [K, 4]: warp_of_crop of every crop (top, left, height, width) of the four lists' product, in that nesting order, that
    lies inside the canvas and whose scale is in the warp's range."""
    H, W = int(canvas_hw[0]), int(canvas_hw[1])
    h, w = int(leak_hw[0]), int(leak_hw[1])
    out = []
    for top in tops:
        for left in lefts:
            for ch in heights:
                for cw in widths:
                    if top < 0 or left < 0 or ch < 1 or cw < 1 or top + ch > H or left + cw > W:
                        continue
                    g = warp_of_crop(top, left, ch, cw, h, w)
                    if WARP_MIN_A <= g[0] <= WARP_MAX_A and WARP_MIN_A <= g[2] <= WARP_MAX_A:
                        out.append(g)
    return np.asarray(out, dtype=np.int64).reshape(-1, 4)


# ---- rotated leaks: the same warp under a 2x3 affine map ------------------------------------------------------------------------
AFFINE_MAX_A, AFFINE_MIN_DET, AFFINE_MAX_B = 1 << 20, 1 << 24, 1 << 48


def _affine_ok(g) -> bool:
    ayy, ayx, by, axy, axx, bx = (int(v) for v in g)
    return (all(abs(a) <= AFFINE_MAX_A for a in (ayy, ayx, axy, axx)) and abs(by) <= AFFINE_MAX_B and abs(bx) <= AFFINE_MAX_B
            and abs(ayy * axx - ayx * axy) >= AFFINE_MIN_DET)


def affine_of_warp(geom4) -> tuple:
    """(ayy, ayx, by, axy, axx, bx) of a warp geometry (ay, by, ax, bx): zero off-diagonal terms, the same warp byte for byte."""
    ay, by, ax, bx = (int(v) for v in np.asarray(geom4).reshape(-1))
    return ay, 0, by, 0, ax, bx


def affine_of_rotation(canvas_hw, leak_hw, angle_deg: float, scale: float = 1.0, shift=(0.0, 0.0)) -> tuple:
    """(ayy, ayx, by, axy, axx, bx), Q16: the map canvas pixel -> leak sample for a leak whose pixel p = (y, x) shows the canvas at
    scale * R(angle) * (p - c_leak) + c_canvas + shift, with R(a) = [[cos a, -sin a], [sin a, cos a]] on (y, x) vectors and c the
    index centres ((H - 1) / 2, (W - 1) / 2).  It is the inverse map, p = R(-angle) / scale * (q - c_canvas - shift) + c_leak,
    each coefficient rounded once to Q16 (float64, to nearest); the integers are the definition from there on."""
    a = np.deg2rad(float(angle_deg))
    m = np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]]) / float(scale)
    cl = np.array([(int(leak_hw[0]) - 1) / 2.0, (int(leak_hw[1]) - 1) / 2.0])
    cc = np.array([(int(canvas_hw[0]) - 1) / 2.0 + float(shift[0]), (int(canvas_hw[1]) - 1) / 2.0 + float(shift[1])])
    b = cl - m @ cc
    q = [int(np.rint(v * WARP_ONE)) for v in (m[0, 0], m[0, 1], b[0], m[1, 0], m[1, 1], b[1])]
    return tuple(q)


def affine_units(leak_hw, canvas_hw, geom) -> np.ndarray:
    """bool [H // 8, W // 8]: the canvas units whose 64 pixels all fall inside the leak under the affine ``geom``.  Positions are
    affine and the inside set is an intersection of half-planes, so a unit counts iff its four corner pixels are inside; the
    counting units are convex, not a rectangle.  Bounding rectangle and count equal the library's ofmk_affine_units."""
    g = tuple(int(v) for v in np.asarray(geom).reshape(-1))
    if len(g) != 6 or not _affine_ok(g):
        raise ValueError("an affine geometry is (ayy, ayx, by, axy, axx, bx) with coefficients in [-2^20, 2^20], |b| <= 2^48 and "
                         "|ayy * axx - ayx * axy| >= 2^24")
    ayy, ayx, by, axy, axx, bx = g
    h, w = int(leak_hw[0]), int(leak_hw[1])
    i = 8 * np.arange(int(canvas_hw[0]) // 8, dtype=np.int64)[:, None]
    j = 8 * np.arange(int(canvas_hw[1]) // 8, dtype=np.int64)[None, :]
    ok = np.ones((i.shape[0], j.shape[1]), bool)
    for dy in (0, 7):
        for dx in (0, 7):
            y0, x0 = (ayy * (i + dy) + ayx * (j + dx) + by) >> 16, (axy * (i + dy) + axx * (j + dx) + bx) >> 16
            ok &= (y0 >= 0) & (y0 <= h - 1) & (x0 >= 0) & (x0 <= w - 1)
    return ok


def rotation_candidates(canvas_hw, leak_hw, angles, scales, shifts_y, shifts_x) -> np.ndarray:
    """int64 [K, 6]: affine_of_rotation of every (angle, scale, shift_y, shift_x) of the four lists' product, in that nesting
    order, whose map is in the affine warp's range."""
    out = []
    for angle in angles:
        for scale in scales:
            for sy in shifts_y:
                for sx in shifts_x:
                    g = affine_of_rotation(canvas_hw, leak_hw, angle, scale, (sy, sx))
                    if _affine_ok(g):
                        out.append(g)
    return np.asarray(out, dtype=np.int64).reshape(-1, 6)


def _geometries(geometries) -> np.ndarray:
    """int64 [K, 4] warp geometries or [K, 6] affine ones (a single geometry of six numbers is [1, 6])."""
    g = np.asarray(_host(geometries), dtype=np.int64)
    return g.reshape(-1, 6) if g.shape[-1:] == (6,) else g.reshape(-1, 4)


def best_geometry(scores, cands, leak_hw, canvas_hw) -> dict:
    """scores: [K] or [n, K] sums of |soft metric| per candidate geometry (rows are added); cands: int64 [K, 4] (or [K, 6] affine
    geometries: units from affine_units) ->
    dict(index, geometry=(ay, by, ax, bx), normalised=float64 [K], contrast=top / second).  normalised = score / (2^14 * counting
    units * frames): about 0.8 at a marked leak's true geometry (bilinear resampling twice costs the rest), the unmarked level
    (0.6-0.7) elsewhere; candidates without a counting unit are excluded (0 there).  No verdict: the caller judges ``contrast``
    (inf when one candidate at most has units or the second-best scores 0)."""
    cands = _geometries(cands)
    K = cands.shape[0]
    s = np.asarray(scores, dtype=np.int64).reshape(-1, K)
    units = np.empty(K, np.int64)
    for k in range(K):
        if cands.shape[1] == 6:
            units[k] = int(affine_units(leak_hw, canvas_hw, cands[k]).sum())
            continue
        i0, i1, j0, j1 = warp_units(leak_hw, canvas_hw, cands[k])
        units[k] = (i1 - i0) * (j1 - j0)
    have = units > 0
    if not have.any():
        raise ValueError("no candidate geometry has a counting unit")
    norm, top, contrast = _rank(s, units, have)
    return dict(index=top, geometry=tuple(int(v) for v in cands[top]), normalised=norm, contrast=contrast)


def read_rescaled_leak(decoder, frames, segment_of_frame, canvas_hw, candidates, geometries, key=0, L: int = 8, search_frames: int = 8) -> dict:
    """A rescaled (cropped and / or resized) leak's copy per segment.  decoder: a DwtDctSvdDecoder (blk 4) or a DctDecoder
    (anything with their decode_soft_warp_u8); frames: CUDA uint8 [n, h, w, 3], the leak as it is; canvas_hw: the marked
    (uncropped) frames' (H, W); candidates: per segment the payloads it may carry, as read_cropped_leak; geometries: int64 [K, 4]
    warp geometries (crop_candidates / warp_of_crop).  With K > 1 the first ``search_frames`` frames are scored under every
    geometry (decoder.warp_scores_u8: DwtDctSvdDecoder only -- ValueError otherwise) and best_geometry picks one; with K = 1
    nothing is searched.  All frames are then read at that geometry, summed per segment, and each segment takes the candidate
    that correlates best with the position rotation fixed at 0 (canvas coordinates leave none).  -> dict(geometry, index,
    contrast, normalised (None, None without a search), segments, soft_by_segment, base (0), picks, score, runner_up_score
    (None), ambiguous).  No verdict on ``contrast``.
    ``geometries`` may also be int64 [K, 6] affine geometries (rotation_candidates / affine_of_rotation): the search is then
    decoder.affine_scores_u8, the read-out decoder.decode_soft_affine_u8 and the units come from affine_units.  Only
    DwtDctSvdDecoder has them: a DctDecoder with a 6-column geometry raises ValueError."""
    leak_hw = (int(frames.shape[1]), int(frames.shape[2]))
    canvas_hw = (int(canvas_hw[0]), int(canvas_hw[1]))
    geoms = _geometries(geometries)
    if geoms.shape[0] < 1:
        raise ValueError("geometries must hold at least one (ay, by, ax, bx)")
    affine = geoms.shape[1] == 6
    search, read = ("affine_scores_u8", "decode_soft_affine_u8") if affine else ("warp_scores_u8", "decode_soft_warp_u8")
    if affine and not hasattr(decoder, read):
        raise ValueError(f"{type(decoder).__name__} does not read at an affine geometry ({read}): only DwtDctSvd does")
    if geoms.shape[0] > 1:
        if not hasattr(decoder, search):
            raise ValueError(f"{type(decoder).__name__} has no geometry search ({search}): give the one known geometry")
        found = best_geometry(_host(getattr(decoder, search)(frames[:max(1, int(search_frames))], canvas_hw, geoms)), geoms, leak_hw, canvas_hw)
    else:
        found = dict(index=0, geometry=tuple(int(v) for v in geoms[0]), normalised=None, contrast=None)
    soft = getattr(decoder, read)(frames, canvas_hw, found["geometry"], L)
    out = _align_by_segment(soft, segment_of_frame, candidates, key, bases=(0,))
    out.update(geometry=found["geometry"], index=found["index"], contrast=found["contrast"], normalised=found["normalised"])
    return out


# ---- rotated (or rescaled) AND cropped leaks: the translation leaves the candidate list ---------------------------------------------
def shift_affine(geom, py: int, px: int):
    """g (+) (py, px): the affine geometry that reads, at canvas pixel (y, x), what ``geom`` reads at canvas pixel (y + py, x + px) --
    by' = by + ayy * py + ayx * px, bx' = bx + axy * py + axx * px, exact in Python integers.  One geometry of six -> a tuple of six
    ints; an int64 [K, 6] array -> an int64 [K, 6] array."""
    g = np.asarray(_host(geom))
    py, px = int(py), int(px)

    def one(v):
        ayy, ayx, by, axy, axx, bx = (int(c) for c in v)
        return ayy, ayx, by + ayy * py + ayx * px, axy, axx, bx + axy * py + axx * px

    if g.ndim == 1 and g.size == 6:
        return one(g)
    if g.ndim != 2 or g.shape[1] != 6:
        raise ValueError("an affine geometry is (ayy, ayx, by, axy, axx, bx), or an int64 [K, 6] array of them")
    return np.asarray([one(v) for v in g], dtype=np.int64).reshape(-1, 6)


def subpixel_shifts(s: int = 2) -> tuple:
    """(0, 1/s, ..., (s - 1)/s): the shifts in [0, 1) px of one axis; given to rotation_candidates as both ``shifts_y`` and
    ``shifts_x`` they make the s x s sub-pixel lattice the dense shift search needs on top of its 64 whole-pixel phases.  Module
    docstring: whole pixels alone (s = 1) are not enough; s = 2 reads whole-pixel crops of a frame rotated about its centre; the
    score's peak is about a quarter of a pixel wide, so an arbitrary translation takes s = 8."""
    s = int(s)
    if s < 1:
        raise ValueError("s must be at least 1")
    return tuple(k / s for k in range(s))


def best_shifted_geometry(scores, units, cands) -> dict:
    """scores: [K, 64] or [n, K, 64] sums of |soft metric| per candidate and whole-pixel shift (rows are added); units: [K, 64]
    counting units behind each entry (both from decoder.affine_phase_scores_u8); cands: int64 [K, 6] ->
    dict(index, phase=(py, px), geometry = shift_affine(cands[index], py, px), normalised=float64 [K, 64] = score / (2^14 * units *
    frames), 0 where units is 0; contrast = best / the best entry of any OTHER candidate; phase_contrast = best / the second-best
    phase of the SAME candidate; each inf when there is no such entry or it scores 0).  No verdict: the caller judges the two
    contrasts (about 1.05 and 1.07-1.09 on four small frames of the test recipe: thin)."""
    cands = _geometries(cands)
    K = cands.shape[0]
    if cands.shape[1] != 6:
        raise ValueError("cands must be int64 [K, 6] affine geometries")
    s = np.asarray(_host(scores), dtype=np.int64).reshape(-1, K * 64)
    u = np.asarray(_host(units), dtype=np.int64).reshape(K * 64)
    have = u > 0
    if not have.any():
        raise ValueError("no candidate geometry has a counting unit under any shift")
    norm, top, _ = _rank(s, u, have)
    norm = norm.reshape(K, 64)
    index, phase = top // 64, ((top % 64) // 8, top % 8)

    def over(rest):
        return float(norm[index, top % 64] / rest.max()) if rest.size and rest.max() > 0 else float("inf")

    return dict(index=index, phase=phase, geometry=shift_affine(cands[index], *phase), normalised=norm,
                contrast=over(np.delete(norm, index, axis=0)), phase_contrast=over(np.delete(norm[index], top % 64)))


def read_transformed_leak(decoder, frames, segment_of_frame, canvas_hw, candidates, geometries, key=0, L: int = 8, search_frames: int = 8) -> dict:
    """A rotated (or rescaled) AND cropped leak's copy per segment: the translation is not known.  decoder: a DwtDctSvdDecoder
    (blk 4; anything with its affine_phase_scores_u8 / decode_soft_affine_u8 -- a DctDecoder raises ValueError); frames: CUDA
    uint8 [n, h, w, 3], the leak as it is; canvas_hw, candidates, key, L: as read_rescaled_leak; geometries: int64 [K, 6], the
    LINEAR parts to try, each with the sub-pixel shifts to try (rotation_candidates(..., subpixel_shifts(2), subpixel_shifts(2))) --
    whole-pixel translations need no entries.
      1. the first ``search_frames`` frames are scored under every geometry and all 64 whole-pixel shifts of the canvas
         (decoder.affine_phase_scores_u8) and best_shifted_geometry picks one shifted geometry;
      2. all frames are read at it (decoder.decode_soft_affine_u8) and summed per segment;
      3. shifts by whole units are left: they rotate the L positions by a constant, which align_segments resolves over all L bases.
    -> dict(index, phase, geometry (the shifted one), normalised, contrast, phase_contrast, segments, soft_by_segment, base, picks,
    score, runner_up_score, ambiguous).  No verdict on the contrasts."""
    canvas_hw = (int(canvas_hw[0]), int(canvas_hw[1]))
    geoms = _geometries(geometries)
    if geoms.shape[0] < 1 or geoms.shape[1] != 6:
        raise ValueError("geometries must hold at least one (ayy, ayx, by, axy, axx, bx)")
    for need in ("affine_phase_scores_u8", "decode_soft_affine_u8"):
        if not hasattr(decoder, need):
            raise ValueError(f"{type(decoder).__name__} does not read at an affine geometry ({need}): only DwtDctSvd does")
    scores, units = decoder.affine_phase_scores_u8(frames[:max(1, int(search_frames))], canvas_hw, geoms)
    found = best_shifted_geometry(scores, units, geoms)
    soft = decoder.decode_soft_affine_u8(frames, canvas_hw, found["geometry"], L)
    out = _align_by_segment(soft, segment_of_frame, candidates, key)
    out.update(found)
    return out


# ---- leaks read against their SOURCE frames: registration in place of a geometry list ------------------------------------------------
ALIGN_SUMS = 29               # per frame and candidate: 21 of sum sd sd^T (upper triangle, row-major), 6 of sum sd e, sum e^2, the count
ALIGN_MIN_PIXELS = 384        # fewer contributing pixels than this give no step
ALIGN_MAX_SIDE = 4096         # canvas H, W: keeps a frame's sums inside int64


class NoAlignStep(ValueError):
    """align_step has no step to give; the message says why."""


def level_down(geom) -> tuple:
    """The geometry one pyramid level up (both the canvas and the leak halved by the 2x2 box, odd last row / column dropped): level
    l + 1 pixel P sits at level-l coordinate 2 P + 1/2, so the linear part stays and by' = (by + (ayy + ayx) / 2 - 2^15) / 2, bx alike,
    each rounded once to Q16 (exact integers, halves up)."""
    ayy, ayx, by, axy, axx, bx = (int(v) for v in np.asarray(_host(geom)).reshape(-1))
    return ayy, ayx, _round_div(2 * by + ayy + ayx - WARP_ONE, 4), axy, axx, _round_div(2 * bx + axy + axx - WARP_ONE, 4)


def level_up(geom) -> tuple:
    """level_down's inverse: by' = 2 by + 2^15 - (ayy + ayx) / 2, bx alike, each rounded once to Q16.  level_up(level_down(g)) moves no
    sample by more than 2^-16 px per axis (a half down, doubled; when ayy + ayx is odd a quarter down and a half up)."""
    ayy, ayx, by, axy, axx, bx = (int(v) for v in np.asarray(_host(geom)).reshape(-1))
    return ayy, ayx, _round_div(4 * by + WARP_ONE - ayy - ayx, 2), axy, axx, _round_div(4 * bx + WARP_ONE - axy - axx, 2)


def corner_move(g0, g1, canvas_hw) -> float:
    """The largest distance, in leak pixels, between the samples of the four canvas corner pixels under g0 and under g1."""
    a, b = [int(v) for v in g0], [int(v) for v in g1]
    worst = 0.0
    for y in (0, int(canvas_hw[0]) - 1):
        for x in (0, int(canvas_hw[1]) - 1):
            dy = (b[0] - a[0]) * y + (b[1] - a[1]) * x + b[2] - a[2]
            dx = (b[3] - a[3]) * y + (b[4] - a[4]) * x + b[5] - a[5]
            worst = max(worst, float(np.hypot(dy, dx)) / WARP_ONE)
    return worst


def _total_sums(sums) -> list:
    """[..., 29] sums -> 29 Python integers: the frames' sums added without a width."""
    s = np.asarray(_host(sums), dtype=np.int64).reshape(-1, ALIGN_SUMS)
    return [sum(int(v) for v in s[:, i]) for i in range(ALIGN_SUMS)]


def align_step(geom, sums, canvas_hw) -> tuple:
    """One Gauss-Newton step of the leak's geometry towards its source.  sums: int64 [..., 29] of decoder.align_sums_u8 under
    ``geom`` (include/offmark_hip.h: ofmk_align_sums_rgb8), any number of frames; they are added as Python integers.  With Hm the
    6x6 matrix and b the 6-vector of the sums (gradients are TWICE the derivative), d = solve(Hm / 4, b / 2) in float64,
    M = [[d0, d1], [d3, d4]], t = (d2, d5), c = (H >> 1, W >> 1): the warped leak at canvas pixel p looks like the source at
    A(p) = p + M (p - c) + t, so the step is g' = g o A^-1, each coefficient rounded once to Q16.  Raises NoAlignStep when fewer than
    384 pixels contribute or Hm is not positive definite (a flat source: its Cholesky factorisation fails)."""
    g = [int(v) for v in np.asarray(_host(geom)).reshape(-1)]
    if len(g) != 6:
        raise ValueError("an affine geometry is (ayy, ayx, by, axy, axx, bx)")
    tot = _total_sums(sums)
    if tot[28] < ALIGN_MIN_PIXELS:
        raise NoAlignStep(f"{tot[28]} contributing pixels, fewer than {ALIGN_MIN_PIXELS}")
    Hm = np.zeros((6, 6), np.float64)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            Hm[i, j] = Hm[j, i] = float(tot[k]) / 4.0
            k += 1
    b = np.array([float(v) / 2.0 for v in tot[21:27]], np.float64)
    try:
        np.linalg.cholesky(Hm)
    except np.linalg.LinAlgError:
        raise NoAlignStep("the normal matrix is not positive definite (a source without gradients)") from None
    d = np.linalg.solve(Hm, b)
    M = np.array([[d[0], d[1]], [d[3], d[4]]])
    t = np.array([d[2], d[5]])
    c = np.array([float(int(canvas_hw[0]) >> 1), float(int(canvas_hw[1]) >> 1)])
    try:
        inv = np.linalg.inv(np.eye(2) + M)
    except np.linalg.LinAlgError:
        raise NoAlignStep("the step is singular") from None
    lin = np.array([[g[0], g[1]], [g[3], g[4]]], np.float64) @ inv           # g o A^-1: q -> L inv q + L inv (M c - t) + b
    off = lin @ (M @ c - t) + np.array([g[2], g[5]], np.float64)
    vals = (lin[0, 0], lin[0, 1], off[0], lin[1, 0], lin[1, 1], off[1])
    if not all(np.isfinite(v) and abs(v) < 2.0 ** 62 for v in vals):
        raise NoAlignStep("the step is not finite")
    return tuple(int(np.rint(v)) for v in vals)


def default_levels(leak_hw) -> int:
    """Pyramid levels of register_leak, the full resolution included: the leak is halved while its shorter side stays >= 48."""
    side, levels = min(int(leak_hw[0]), int(leak_hw[1])), 1
    while side // 2 >= 48:
        side //= 2
        levels += 1
    return levels


def register_leak(decoder, sources, frames, canvas_hw, start=None, levels=None, max_iters: int = 15, tol_px: float = 1.0 / 64) -> dict:
    """The geometry of a leak from its SOURCE frames, with no list: Gauss-Newton on the luma difference between the warped leak and
    the source, six parameters, coarse to fine.  decoder: a DwtDctSvdDecoder (anything with its align_sums_u8 / halve_u8);
    sources: uint8 [n, H, W, 3], frame i's source on the canvas; frames: uint8 [n, h, w, 3], the leak; start: the first geometry
    (default affine_of_rotation(canvas_hw, leak_hw, 0.0): centred, unrotated); levels: pyramid levels, full resolution included
    (default_levels).  Each level iterates align_step until the four canvas corners move less than ``tol_px`` leak pixels or
    ``max_iters`` steps are taken -- the integer iteration wobbles in its last Q16 bits and has no exact fixed point --, then hands
    level_up of its geometry to the finer level.  -> dict(geometry, iterations (per level, coarse to fine), rms (the luma residual at
    the last geometry that was measured, full resolution), pixels (that measurement's contributing pixels, all frames), units
    (counting units of the geometry), converged (the finest level met ``tol_px``), reason (None, or why not)).  Nothing is raised for a
    leak that cannot be registered: ``converged`` is False and ``reason`` says why."""
    canvas_hw = (int(canvas_hw[0]), int(canvas_hw[1]))
    leak_hw = (int(frames.shape[1]), int(frames.shape[2]))
    if tuple(int(v) for v in sources.shape[:3]) != (int(frames.shape[0]), *canvas_hw):
        raise ValueError("sources must be [n, H, W, 3] with one canvas-sized frame per leak frame")
    g = tuple(int(v) for v in (affine_of_rotation(canvas_hw, leak_hw, 0.0) if start is None else np.asarray(_host(start)).reshape(-1)))
    if len(g) != 6:
        raise ValueError("start must be an affine geometry of six")
    levels = default_levels(leak_hw) if levels is None else int(levels)
    if levels < 1:
        raise ValueError("levels must be at least 1")
    pyramid = [(sources, frames)]
    for _ in range(levels - 1):
        s, f = pyramid[-1]
        pyramid.append((decoder.halve_u8(s), decoder.halve_u8(f)))
        g = level_down(g)
    iterations, reason, met, rms, pixels = [], None, False, None, 0
    for level in range(levels - 1, -1, -1):
        s, f = pyramid[level]
        hw = (int(s.shape[1]), int(s.shape[2]))
        steps, met = 0, False
        while steps < int(max_iters) and reason is None and not met:
            tot = _total_sums(decoder.align_sums_u8(s, f, hw, np.asarray([g], dtype=np.int64)))
            if level == 0:
                pixels = tot[28]
                rms = float(np.sqrt(tot[27] / tot[28])) if tot[28] else None
            try:
                nxt = align_step(g, tot, hw)
                if not _affine_ok(nxt):
                    raise NoAlignStep("the step leaves the affine warp's range")
            except NoAlignStep as exc:
                reason = f"level {level}: {exc}"
                break
            steps += 1
            met = corner_move(g, nxt, hw) < float(tol_px)
            g = nxt
        iterations.append(steps)
        if reason is not None:
            iterations += [0] * level
            for _ in range(level):
                g = level_up(g)
            break
        if level:
            g = level_up(g)
    if reason is None and not met:
        reason = f"level 0: the corners still move by {tol_px} px or more after {max_iters} steps"
    units = int(affine_units(leak_hw, canvas_hw, g).sum()) if _affine_ok(g) else 0
    return dict(geometry=g, iterations=iterations, rms=rms, pixels=pixels, units=units, converged=reason is None, reason=reason)


def read_registered_leak(decoder, frames, sources, segment_of_frame, canvas_hw, candidates, key=0, L: int = 8, search_frames: int = 8,
                         **register) -> dict:
    """A transformed leak's copy per segment, read against its SOURCE frames: no list of geometries.  decoder: a DwtDctSvdDecoder
    (blk 4; anything with its align_sums_u8 / halve_u8 / decode_soft_affine_u8 -- a DctDecoder raises ValueError); frames: uint8
    [n, h, w, 3], the leak; sources: uint8 [n, H, W, 3], sources[i] is frame i's unmarked (or marked) source; the other arguments as
    read_transformed_leak; ``register``: start, levels, max_iters, tol_px of register_leak.
      1. register_leak on the first ``search_frames`` frames and their sources;
      2. all frames are read at that geometry (decoder.decode_soft_affine_u8) and summed per segment;
      3. the geometry lies on the source's own pixel grid, so no rotation of the positions is left: align_segments with bases (0,).
    -> read_transformed_leak's keys (index 0, phase (0, 0), base 0, runner_up_score None; normalised = the geometry's score /
    (2^14 * units * frames) on the search frames where the decoder has affine_scores_u8, else None; contrast and phase_contrast
    None: nothing was ranked) plus ``registration``, register_leak's report.  No verdict: judge ``registration['converged']``."""
    canvas_hw = (int(canvas_hw[0]), int(canvas_hw[1]))
    for need in ("align_sums_u8", "halve_u8", "decode_soft_affine_u8"):
        if not hasattr(decoder, need):
            raise ValueError(f"{type(decoder).__name__} does not read at an affine geometry ({need}): only DwtDctSvd does")
    k = max(1, int(search_frames))
    report = register_leak(decoder, sources[:k], frames[:k], canvas_hw, **register)
    geom = report["geometry"]
    normalised = None
    if hasattr(decoder, "affine_scores_u8") and report["units"] > 0:
        s = _host(decoder.affine_scores_u8(frames[:k], canvas_hw, np.asarray([geom], dtype=np.int64))).astype(np.int64)
        normalised = float(s.sum()) / (float(ONE) * report["units"] * s.shape[0])
    soft = decoder.decode_soft_affine_u8(frames, canvas_hw, geom, L)
    out = _align_by_segment(soft, segment_of_frame, candidates, key, bases=(0,))
    out.update(index=0, phase=(0, 0), geometry=geom, normalised=normalised, contrast=None, phase_contrast=None, registration=report)
    return out
