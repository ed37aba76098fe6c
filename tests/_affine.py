"""Shared by the rotated-leak tests (test_affine_statement.py, test_affine_abi.py, test_gpu_affine.py): the NumPy statement of the
integer affine warp, of the counting units, of the geometry scores and of the read-out, over tests/_warp.py and tests/_svd_soft.py;
a deterministic float64 bilinear rotation "attack"; and the recipe.

Statement (include/offmark_hip.h: ofmk_affine): canvas pixel (y, x) reads the leak (h x w) at pos_y = ayy * y + ayx * x + by,
pos_x = axy * y + axx * x + bx (int64, Q16); from there on tests/_warp.py's rule: c0 = pos >> 16, f = (pos >> 8) & 255, inside iff
0 <= y0 <= h - 1 and 0 <= x0 <= w - 1 -- decided per PIXEL here --, second taps min(c0 + 1, len - 1), the one rounding, 0 outside.
A canvas unit counts iff all 64 of its pixels are inside: from the per-pixel mask, not through the four-corner rule the library
and offmark.resync use.  The score of a geometry is sum |m| over the counting units of the warped canvas; the read-out adds unit
(i, j) into position (i * (W // 8) + j) % L."""
import functools

import numpy as np

import _resync as rs
import _svd_soft as ss
import _warp as wp

ONE = 65536
IDENTITY = (ONE, 0, 0, 0, ONE, 0)


def hflip(w):
    """The horizontal flip: canvas (y, x) reads leak (y, w - 1 - x)."""
    return ONE, 0, 0, 0, -ONE, (w - 1) << 16


def warp(frame, geom, out_hw, origin=(0, 0)):
    """-> (u8 [Hout, Wout, 3], inside bool [Hout, Wout]): the statement of the affine warp of one leak frame."""
    ayy, ayx, by, axy, axx, bx = (int(v) for v in geom)
    h, w = frame.shape[:2]
    y = (np.arange(out_hw[0], dtype=np.int64) + origin[0])[:, None]
    x = (np.arange(out_hw[1], dtype=np.int64) + origin[1])[None, :]
    py, px = ayy * y + ayx * x + by, axy * y + axx * x + bx
    y0, x0 = py >> 16, px >> 16
    inside = (y0 >= 0) & (y0 <= h - 1) & (x0 >= 0) & (x0 <= w - 1)
    y0, x0 = np.where(inside, y0, 0), np.where(inside, x0, 0)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    fy, fx = ((py >> 8) & 255)[:, :, None], ((px >> 8) & 255)[:, :, None]
    p = frame.astype(np.int64)
    top = (256 - fx) * p[y0, x0] + fx * p[y0, x1]
    bot = (256 - fx) * p[y1, x0] + fx * p[y1, x1]
    v = ((256 - fy) * top + fy * bot + 32768) >> 16
    return np.ascontiguousarray(np.where(inside[:, :, None], v, 0).astype(np.uint8)), inside


def units(leak_hw, canvas_hw, geom):
    """bool [H // 8, W // 8]: the units all of whose 64 pixels are inside, from the per-pixel mask of the whole canvas."""
    H8, W8 = canvas_hw[0] // 8, canvas_hw[1] // 8
    _, inside = warp(np.zeros((leak_hw[0], leak_hw[1], 3), np.uint8), geom, (8 * H8, 8 * W8))
    return inside.reshape(H8, 8, W8, 8).all(axis=(1, 3))


def corner_units(leak_hw, canvas_hw, geom):
    """The same from the four corner pixels of every unit only."""
    H8, W8 = canvas_hw[0] // 8, canvas_hw[1] // 8
    _, inside = warp(np.zeros((leak_hw[0], leak_hw[1], 3), np.uint8), geom, (8 * H8, 8 * W8))
    u = inside.reshape(H8, 8, W8, 8)
    return u[:, 0, :, 0] & u[:, 0, :, 7] & u[:, 7, :, 0] & u[:, 7, :, 7]


def rect_and_count(mask):
    """(i0, i1, j0, j1, count) of a unit mask: what ofmk_affine_units returns; all 0 when no unit counts."""
    if not mask.any():
        return 0, 0, 0, 0, 0
    ii, jj = np.flatnonzero(mask.any(axis=1)), np.flatnonzero(mask.any(axis=0))
    return int(ii[0]), int(ii[-1]) + 1, int(jj[0]), int(jj[-1]) + 1, int(mask.sum())


def unit_metrics(frame, canvas_hw, geom, scale=15.0):
    """-> (m int64 [H // 8, W // 8] of the warped canvas, 0 where the unit does not count; the counting mask)."""
    H8, W8 = canvas_hw[0] // 8, canvas_hw[1] // 8
    mask = units(frame.shape[:2], canvas_hw, geom)
    if not mask.any():
        return np.zeros((H8, W8), np.int64), mask
    out, _ = warp(frame, geom, (8 * H8, 8 * W8))
    m = ss.statement(out, scale=scale)["m"].reshape(H8, W8)
    return np.where(mask, m, 0), mask


def statement_score(frame, canvas_hw, geom, scale=15.0):
    return int(np.abs(unit_metrics(frame, canvas_hw, geom, scale)[0]).sum())


def statement_soft(frame, canvas_hw, geom, L, scale=15.0):
    """int64 [L]: the read-out of one leak frame at ``geom``, unit (i, j) at position (i * (W // 8) + j) % L."""
    m, _ = unit_metrics(frame, canvas_hw, geom, scale)
    return ss.regroup(m.reshape(-1), L)


def chain_unit_metrics(eng, dev, canvas, g, scale=15):
    """The chain the fused device calls replace (test_gpu_affine.py, test_gpu_geometry_edges.py): int64 [n, H // 8, W // 8] on the
    host from engine.warp_affine of the whole canvas + svd_detect_soft with one position per unit, masked by the statement's
    counting units."""
    H8, W8 = canvas[0] // 8, canvas[1] // 8
    warped = eng.warp_affine(dev, g, (8 * H8, 8 * W8))
    m = eng.svd_detect_soft(warped, H8 * W8, scale=scale).cpu().numpy().reshape(-1, H8, W8)
    return np.where(units(tuple(dev.shape[1:3]), canvas, g)[None], m, 0)


# ---- the attack: a float64 bilinear rotation (and scale) about the centre, on the host ----------------------------------------
def rotate(frames, angle_deg, step=1.0, out_hw=None):
    """frames u8 [n, H, W, 3] -> u8 [n, h, w, 3], read-only: leak pixel p = (y, x) samples the frame at
    step * R(angle) * (p - c_leak) + c_frame, R(a) = [[cos a, -sin a], [sin a, cos a]] on (y, x), c the index centres; the sample
    coordinates are clamped into the frame; float64 bilinear, rint, clip.  What offmark.resync.affine_of_rotation inverts."""
    H, W = frames.shape[1:3]
    h, w = (H, W) if out_hw is None else out_hw
    a = np.deg2rad(angle_deg)
    dy, dx = np.arange(h, dtype=np.float64)[:, None] - (h - 1) / 2.0, np.arange(w, dtype=np.float64)[None, :] - (w - 1) / 2.0
    sy = np.clip(step * (np.cos(a) * dy - np.sin(a) * dx) + (H - 1) / 2.0, 0.0, H - 1.0)
    sx = np.clip(step * (np.sin(a) * dy + np.cos(a) * dx) + (W - 1) / 2.0, 0.0, W - 1.0)
    y0, x0 = np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    fy, fx = (sy - y0)[None, :, :, None], (sx - x0)[None, :, :, None]
    p = frames.astype(np.float64)
    top = (1 - fx) * p[:, y0, x0] + fx * p[:, y0, x1]
    bot = (1 - fx) * p[:, y1, x0] + fx * p[:, y1, x1]
    out = np.ascontiguousarray(np.clip(np.rint((1 - fy) * top + fy * bot), 0, 255).astype(np.uint8))
    out.setflags(write=False)
    return out


# ---- the recipe: tests/_warp.py's marked 3 segments x 4 frames of 72x104, copies (1, 0, 1), rotated about the centre, same size ---
H, W, S, F, L8, KEY, CHOSEN = wp.H, wp.W, wp.S, wp.F, wp.L8, wp.KEY, wp.CHOSEN
CANVAS = (H, W)
SEARCH_FRAMES = 4
ATTACKS = {"2deg": (2.0, 1.0), "-3deg-step-1.10": (-3.0, 1.10)}      # angle in degrees, step


@functools.lru_cache(maxsize=None)
def leak(codec, attack="2deg"):
    """codec "svd": the oracle-marked recipe attacked; "none": the unmarked sources attacked the same way.  u8 [12, 72, 104, 3]."""
    return rotate(rs.recipe_sources() if codec == "none" else wp.marked("svd"), *ATTACKS[attack])


def candidate_parameters(attack="2deg"):
    """35 (angle, scale, shift_y, shift_x): the true one first, then the angle off by 0.25 / 0.5 / 0.75 degrees either way, the 24
    shifts by (dy, dx) in -2..2 px, and the scale off by 1 and 2 % either way."""
    angle, step = ATTACKS[attack]
    out = [(angle, step, 0.0, 0.0)]
    out += [(angle + d, step, 0.0, 0.0) for d in (-0.75, -0.5, -0.25, 0.25, 0.5, 0.75)]
    out += [(angle, step, float(dy), float(dx)) for dy in range(-2, 3) for dx in range(-2, 3) if (dy, dx) != (0, 0)]
    out += [(angle, step * s, 0.0, 0.0) for s in (0.98, 0.99, 1.01, 1.02)]
    return out


def candidate_geometries(attack="2deg"):
    """int64 [35, 6]; index 0 is the true geometry."""
    from offmark import resync
    return np.asarray([resync.affine_of_rotation(CANVAS, CANVAS, a, s, (dy, dx)) for a, s, dy, dx in candidate_parameters(attack)], dtype=np.int64)


class StatementDecoder:
    """DwtDctSvdDecoder's rotated-leak methods over the statement, on host arrays: what offmark.resync.read_rescaled_leak drives."""

    def affine_scores_u8(self, frames, canvas_hw, cands):
        return np.asarray([[statement_score(f, canvas_hw, g) for g in np.asarray(cands)] for f in frames], dtype=np.int64)

    def decode_soft_affine_u8(self, frames, canvas_hw, geom, L):
        return np.stack([statement_soft(f, canvas_hw, geom, L) for f in frames])
