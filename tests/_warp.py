"""Shared by the rescaled-leak tests (test_warp_statement.py, test_warp_abi.py, test_gpu_warp.py): the NumPy statement of the
integer warp, of the counting units, of the geometry scores and of the read-out, over tests/_svd_soft.py's statement of the unit
metric (DwtDctSvd) and tests/_dct_resync.py's block_metric (DCT); the recipe; and a deterministic float64 bilinear "attack".

Statement (include/offmark_hip.h: ofmk_warp): canvas pixel (y, x) reads the leak (h x w) at pos_y = ay * y + by, pos_x = ax * x + bx
(int64, Q16): y0 = pos_y >> 16, fy = (pos_y >> 8) & 255, inside iff 0 <= y0 <= h - 1 (columns alike), second taps min(y0 + 1, h - 1),
    v = ((256 - fy) * ((256 - fx) * p00 + fx * p01) + fy * ((256 - fx) * p10 + fx * p11) + 32768) >> 16,   0 outside.
A canvas unit counts iff all 64 of its pixels are inside -- decided here per pixel, not through the monotone-map shortcut the
library and offmark.resync use.  The score of a geometry is sum |m| over the counting units of the warped canvas; the read-out adds
unit (i, j) into position (i * (W // 8) + j) % L."""
import functools

import numpy as np

import _dct_resync as dr
import _resync as rs
import _svd_soft as ss

IDENTITY = (65536, 0, 65536, 0)


def _taps(a, b, count, origin, length):
    pos = a * (np.arange(count, dtype=np.int64) + origin) + b
    c0 = pos >> 16
    inside = (c0 >= 0) & (c0 <= length - 1)
    c0 = np.where(inside, c0, 0)
    return c0, np.minimum(c0 + 1, length - 1), (pos >> 8) & 255, inside


def warp(frame, geom, out_hw, origin=(0, 0)):
    """-> (u8 [Hout, Wout, 3], inside bool [Hout, Wout]): the statement of the warp of one leak frame."""
    ay, by, ax, bx = (int(v) for v in geom)
    h, w = frame.shape[:2]
    y0, y1, fy, in_y = _taps(ay, by, out_hw[0], origin[0], h)
    x0, x1, fx, in_x = _taps(ax, bx, out_hw[1], origin[1], w)
    p = frame.astype(np.int64)
    fy, fx = fy[:, None, None], fx[None, :, None]
    top = (256 - fx) * p[y0][:, x0] + fx * p[y0][:, x1]
    bot = (256 - fx) * p[y1][:, x0] + fx * p[y1][:, x1]
    v = ((256 - fy) * top + fy * bot + 32768) >> 16
    inside = in_y[:, None] & in_x[None, :]
    return np.ascontiguousarray(np.where(inside[:, :, None], v, 0).astype(np.uint8)), inside


def units(leak_hw, canvas_hw, geom):
    """(i0, i1, j0, j1) from the per-pixel inside mask of the whole canvas; (0, 0, 0, 0) when no unit counts."""
    H8, W8 = canvas_hw[0] // 8, canvas_hw[1] // 8
    if H8 < 1 or W8 < 1:
        return 0, 0, 0, 0
    _, inside = warp(np.zeros((leak_hw[0], leak_hw[1], 3), np.uint8), geom, (8 * H8, 8 * W8))
    ok = inside.reshape(H8, 8, W8, 8).all(axis=(1, 3))
    if not ok.any():
        return 0, 0, 0, 0
    ii, jj = np.flatnonzero(ok.any(axis=1)), np.flatnonzero(ok.any(axis=0))
    i0, i1, j0, j1 = int(ii[0]), int(ii[-1]) + 1, int(jj[0]), int(jj[-1]) + 1
    assert ok[i0:i1, j0:j1].all() and ok.sum() == (i1 - i0) * (j1 - j0)      # a rectangle: the maps are monotone
    return i0, i1, j0, j1


def counting_rectangle(frame, canvas_hw, geom):
    """The warped pixels of the counting units, u8 [8 rows, 8 cols, 3], and (i0, i1, j0, j1); (None, zeros) when no unit counts."""
    r = units(frame.shape[:2], canvas_hw, geom)
    if r[1] == r[0]:
        return None, r
    out, inside = warp(frame, geom, (8 * (r[1] - r[0]), 8 * (r[3] - r[2])), origin=(8 * r[0], 8 * r[2]))
    assert inside.all()
    return out, r


def unit_metrics(frame, canvas_hw, geom, codec="svd", scale=15.0):
    """-> (m int64 [rows * cols] row-major over the counting rectangle, (i0, i1, j0, j1)); (empty, zeros) when no unit counts."""
    rect, r = counting_rectangle(frame, canvas_hw, geom)
    if rect is None:
        return np.zeros(0, np.int64), r
    m = ss.statement(rect, scale=scale)["m"] if codec == "svd" else dr.block_metric(rect)
    return m, r


def statement_score(frame, canvas_hw, geom, scale=15.0):
    m, _ = unit_metrics(frame, canvas_hw, geom, "svd", scale)
    return int(np.abs(m).sum())


def statement_soft(frame, canvas_hw, geom, L, codec="svd", scale=15.0):
    """int64 [L]: the read-out of one leak frame at ``geom``, unit (i, j) at position (i * (W // 8) + j) % L."""
    m, (i0, i1, j0, j1) = unit_metrics(frame, canvas_hw, geom, codec, scale)
    if m.size == 0:
        return np.zeros(L, np.int64)
    cw = canvas_hw[1] // 8
    return rs.canvas_regroup(m, i1 - i0, j1 - j0, cw, i0 * cw + j0, L)


# ---- the attack: float64 bilinear resize with half-pixel centres, on the host -------------------------------------------------
def resize(frame, out_hw):
    """u8 [h, w, 3]: output pixel y samples the input at (y + 0.5) * H / h - 0.5, clamped into the frame; float64, rint, clip."""
    H, W = frame.shape[:2]
    h, w = out_hw

    def axis(n_in, n_out):
        s = np.clip((np.arange(n_out, dtype=np.float64) + 0.5) * n_in / n_out - 0.5, 0.0, n_in - 1.0)
        c0 = np.floor(s).astype(np.int64)
        return c0, np.minimum(c0 + 1, n_in - 1), s - c0

    y0, y1, fy = axis(H, h)
    x0, x1, fx = axis(W, w)
    p = frame.astype(np.float64)
    fy, fx = fy[:, None, None], fx[None, :, None]
    top = (1 - fx) * p[y0][:, x0] + fx * p[y0][:, x1]
    bot = (1 - fx) * p[y1][:, x0] + fx * p[y1][:, x1]
    return np.clip(np.rint((1 - fy) * top + fy * bot), 0, 255).astype(np.uint8)


def attack(frames, crop, out_hw):
    """frames u8 [n, H, W, 3]; crop = (top, left, ch, cw) -> u8 [n, h, w, 3], read-only."""
    top, left, ch, cw = crop
    out = np.ascontiguousarray(np.stack([resize(f[top:top + ch, left:left + cw], out_hw) for f in frames]))
    out.setflags(write=False)
    return out


# ---- the recipe: tests/_resync.py's 3 segments x 4 frames of 72x104, copies (1, 0, 1); the leak is canvas rows 5:67 / columns
# 7:99 (62 x 92) resized back to 72x104 (zoom back) or down to 54x80 ----
H, W, S, F, L8, KEY = rs.H, rs.W, rs.S, rs.F, rs.L8, rs.KEY
CHOSEN = rs.CHOSEN
CROP = (5, 7, 62, 92)
ZOOM_HW, DOWN_HW = (72, 104), (54, 80)
SEARCH_FRAMES = 4


def true_geometry(leak_hw=ZOOM_HW):
    from offmark import resync
    return resync.warp_of_crop(*CROP, *leak_hw)


def candidate_crops():
    """50 crops: the true one first, then 49 with a crop edge off by 1 or 2 px -- the 24 shifts of the crop by (dt, dl) in
    -2..2 (same size), the 24 size changes (dh, dw) in -2..2 (same top-left corner), and the crop shrunk by 1 px on every side."""
    top, left, ch, cw = CROP
    d = [(a, b) for a in range(-2, 3) for b in range(-2, 3) if (a, b) != (0, 0)]
    return [CROP] + [(top + a, left + b, ch, cw) for a, b in d] + [(top, left, ch + a, cw + b) for a, b in d] + [(top + 1, left + 1, ch - 2, cw - 2)]


def candidate_geometries(leak_hw=ZOOM_HW):
    """int64 [50, 4]; index 0 is the true geometry."""
    from offmark import resync
    return np.asarray([resync.warp_of_crop(*c, *leak_hw) for c in candidate_crops()], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def marked(codec):
    """The recipe marked by the oracle: u8 [12, 72, 104, 3], read-only."""
    src, pay = rs.recipe_sources(), rs.recipe_payloads()
    mark = rs.oracle_mark if codec == "svd" else dr.oracle_mark
    out = np.stack([mark(src[s * F + f], pay[s], KEY) for s in range(S) for f in range(F)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def leak(codec, leak_hw=ZOOM_HW):
    """codec "svd" / "dct": the oracle-marked recipe attacked; "none": the unmarked sources attacked the same way."""
    return attack(rs.recipe_sources() if codec == "none" else marked(codec), CROP, leak_hw)


class StatementDecoder:
    """The decoders' rescaled-leak methods over the statement, on host arrays: what offmark.resync.read_rescaled_leak drives."""

    def __init__(self, codec, search=True):
        self.codec = codec
        if search:
            self.warp_scores_u8 = self._warp_scores

    def _warp_scores(self, frames, canvas_hw, cands):
        return np.asarray([[statement_score(f, canvas_hw, g) for g in np.asarray(cands)] for f in frames], dtype=np.int64)

    def decode_soft_warp_u8(self, frames, canvas_hw, geom, L):
        return np.stack([statement_soft(f, canvas_hw, geom, L, self.codec) for f in frames])
