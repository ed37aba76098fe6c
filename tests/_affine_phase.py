"""Shared by the rotated-and-cropped-leak tests (test_affine_phase_statement.py, test_affine_phase_abi.py, test_gpu_affine_phase.py):
the NumPy statement of the dense shift search over tests/_affine.py, the two leaks of the evidence, and a StatementDecoder.

Statement (include/offmark_hip.h: ofmk_svd_affine_phase_scores_rgb8): scores[k][8 py + px] is tests/_affine.py's statement_score of
the frame under offmark.resync.shift_affine(cands[k], py, px) on the same canvas, units[k][8 py + px] the number of that geometry's
counting units from the per-pixel mask -- 64 separate warps of the whole canvas per candidate, nothing shared between them.  A
candidate that is out of ofmk_affine's range under any of its 64 shifts has zeros throughout."""
import functools

import numpy as np

import _affine as af
import _resync as rs

CANVAS = af.CANVAS
ANGLE = 2.0
SEARCH_FRAMES = af.SEARCH_FRAMES
TRUE_PHASE = (1, 2)
# rows / columns cut out of the recipe rotated by 2 degrees (72 x 104), and the sub-pixel shift of the true geometry: B's odd
# sizes move the leak's index centre by half a pixel
LEAKS = {"A": ((7, 63), (5, 95), (0.0, 0.0)), "A2": ((3, 63), (11, 91), (0.0, 0.0)), "B": ((7, 64), (5, 96), (0.5, 0.5))}


def in_range(geom):
    from offmark import resync
    return all(resync._affine_ok(resync.shift_affine(geom, py, px)) for py in (0, 7) for px in (0, 7))


def statement(frame, canvas_hw, geom, scale=15.0):
    """-> (scores int64 [64], units int64 [64]) of one leak frame under one candidate."""
    from offmark import resync
    scores, units = np.zeros(64, np.int64), np.zeros(64, np.int64)
    if not in_range(geom):
        return scores, units
    for py in range(8):
        for px in range(8):
            g = resync.shift_affine(geom, py, px)
            m, mask = af.unit_metrics(frame, canvas_hw, g, scale)               # statement_score and units of one warp
            scores[8 * py + px], units[8 * py + px] = int(np.abs(m).sum()), int(mask.sum())
    return scores, units


def statement_budget(frame, canvas_hw, geom, scale=15.0):
    """int64 [64]: how far a device score may be from ``statement``'s -- the summed tests/_svd_soft.py unit_budget (two float32 s0 of
    the same block, the project's bound) of the counting units of each shifted geometry."""
    from offmark import resync
    budget = np.zeros(64, np.int64)
    H8, W8 = canvas_hw[0] // 8, canvas_hw[1] // 8
    if not in_range(geom):
        return budget
    for py in range(8):
        for px in range(8):
            g = resync.shift_affine(geom, py, px)
            mask = af.units(frame.shape[:2], canvas_hw, g)
            if mask.any():
                s0 = af.ss.statement(af.warp(frame, g, (8 * H8, 8 * W8))[0], scale=scale)["s0"].reshape(H8, W8)
                budget[8 * py + px] = int(af.ss.unit_budget(s0[mask], scale).sum())
    return budget


def one_warp_statement(frame, canvas_hw, geom, scale=15.0):
    """The same two arrays from ONE warp of the canvas grown by 7 pixels, read at the 64 origins (test_affine_phase_statement.py
    holds shift_affine against the warp's origin, and this against ``statement``): seven times faster, for the searches of the
    CPU tests.  The device is held against ``statement``."""
    scores, units = np.zeros(64, np.int64), np.zeros(64, np.int64)
    if not in_range(geom):
        return scores, units
    H8, W8 = canvas_hw[0] // 8, canvas_hw[1] // 8
    out, inside = af.warp(frame, geom, (8 * H8 + 7, 8 * W8 + 7))
    for py in range(8):
        for px in range(8):
            mask = inside[py:py + 8 * H8, px:px + 8 * W8].reshape(H8, 8, W8, 8).all(axis=(1, 3))
            units[8 * py + px] = int(mask.sum())
            if mask.any():
                m = af.ss.statement(np.ascontiguousarray(out[py:py + 8 * H8, px:px + 8 * W8]), scale=scale)["m"].reshape(H8, W8)
                scores[8 * py + px] = int(np.abs(np.where(mask, m, 0)).sum())
    return scores, units


def statement_scores(frames, canvas_hw, cands, scale=15.0, one=statement):
    """-> (scores int64 [n, K, 64], units int64 [K, 64])."""
    per = [[one(f, canvas_hw, tuple(int(v) for v in g), scale) for g in np.asarray(cands)] for f in frames]
    return np.asarray([[s for s, _ in row] for row in per], dtype=np.int64), np.asarray([u for _, u in per[0]], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def leak(codec, which="A"):
    """codec "svd": the oracle-marked recipe rotated by 2 degrees and cropped; "none": the unmarked sources attacked the same way.
    u8 [12, h, w, 3], read-only."""
    (r0, r1), (c0, c1), _ = LEAKS[which]
    out = np.ascontiguousarray(af.leak(codec, "2deg")[:, r0:r1, c0:c1])
    out.setflags(write=False)
    return out


def leak_hw(which):
    (r0, r1), (c0, c1), _ = LEAKS[which]
    return r1 - r0, c1 - c0


def geometry(which, angle=ANGLE, scale=1.0, shift=(0.0, 0.0)):
    from offmark import resync
    return resync.affine_of_rotation(CANVAS, leak_hw(which), angle, scale, shift)


def candidates(which):
    """The lists of the evidence, int64 [K, 6]; index 0 is the truth.  A: 5 angles at scale 1 and 2 scales at 2 degrees, no
    sub-pixel shift.  B: 3 angles x offmark.resync.subpixel_shifts(2) squared, the truth (2 degrees, (0.5, 0.5)) first."""
    from offmark import resync
    if which.startswith("A"):
        params = [(a, 1.0, (0.0, 0.0)) for a in (2.0, 1.5, 1.75, 2.25, 2.5)] + [(2.0, s, (0.0, 0.0)) for s in (0.99, 1.01)]
    else:
        sub = resync.subpixel_shifts(2)
        params = [(a, 1.0, (sy, sx)) for a in (2.0, 1.75, 2.25) for sy in sub for sx in sub]
        params.insert(0, params.pop(params.index((2.0, 1.0, LEAKS["B"][2]))))
    return np.asarray([geometry(which, a, s, sh) for a, s, sh in params], dtype=np.int64)


def whole_pixel_candidates(which="B"):
    """Leak B's list without the sub-lattice: the three angles at sub-pixel shift (0, 0)."""
    return np.asarray([geometry(which, a) for a in (2.0, 1.75, 2.25)], dtype=np.int64)


class StatementDecoder:
    """DwtDctSvdDecoder's methods that offmark.resync.read_transformed_leak drives, over the statement, on host arrays.  The search
    results are kept per (frames, candidates): several tests ask for the same ones."""
    _cache = {}

    def affine_phase_scores_u8(self, frames, canvas_hw, cands):
        frames, cands = np.asarray(frames), np.asarray(cands, dtype=np.int64)
        key = (frames.shape, frames.tobytes(), tuple(canvas_hw), cands.tobytes())
        if key not in self._cache:
            self._cache[key] = statement_scores(frames, canvas_hw, cands, one=one_warp_statement)
        s, u = self._cache[key]
        return s.copy(), u.copy()

    def decode_soft_affine_u8(self, frames, canvas_hw, geom, L):
        return np.stack([af.statement_soft(f, canvas_hw, geom, L) for f in frames])


def read(decoder, frames, cands, search_frames=SEARCH_FRAMES):
    from offmark import resync
    return resync.read_transformed_leak(decoder, frames, rs.recipe_segments(), CANVAS, rs.recipe_candidates(), cands, key=af.KEY, L=af.L8,
                                        search_frames=search_frames)
