"""Shared by the registration tests (test_align_statement.py, test_gpu_align.py): the NumPy statement of the 29 alignment sums and of
the 2x2 halving over tests/_affine.py's warp, and a StatementDecoder for offmark.resync.register_leak / read_registered_leak.

Statement (include/offmark_hip.h: ofmk_align_sums_rgb8), all integers.  Y = (R + 2 G + B + 2) >> 2.  T = Y of the source frame on the
canvas H x W; Yw = Y of tests/_affine.py's warp of the leak frame under the geometry.  gy = T[y + 1, x] - T[y - 1, x],
gx = T[y, x + 1] - T[y, x - 1] (twice the derivative).  Canvas pixel (y, x) contributes iff 1 <= y <= H - 2, 1 <= x <= W - 2 and the
warp's per-pixel ``inside`` holds.  With yc = y - (H >> 1), xc = x - (W >> 1), sd = (gy yc, gy xc, gy, gx yc, gx xc, gx) and
e = Yw - T, the 29 sums over the contributing pixels are: [0..20] the upper triangle of sum sd sd^T, row-major; [21..26] sum sd e;
[27] sum e^2; [28] the count.  A geometry out of ofmk_affine's range gives 29 zeros.
Halving: out[Y, X, c] = (in[2Y, 2X, c] + in[2Y, 2X + 1, c] + in[2Y + 1, 2X, c] + in[2Y + 1, 2X + 1, c] + 2) >> 2; an odd last row or
column is dropped."""
import numpy as np

import _affine as af

NSUMS = 29


def luma(rgb):
    p = np.asarray(rgb).astype(np.int64)
    return (p[..., 0] + 2 * p[..., 1] + p[..., 2] + 2) >> 2


def sums(source, frame, geom):
    """int64 [29] of one source frame (u8 [H, W, 3]) and one leak frame (u8 [h, w, 3]) under one geometry."""
    from offmark import resync
    out = np.zeros(NSUMS, np.int64)
    g = tuple(int(v) for v in geom)
    if not resync._affine_ok(g):
        return out
    H, W = source.shape[:2]
    T = luma(source)
    warped, inside = af.warp(np.asarray(frame), g, (H, W))
    e = luma(warped) - T
    gy, gx = np.zeros_like(T), np.zeros_like(T)
    gy[1:-1] = T[2:] - T[:-2]
    gx[:, 1:-1] = T[:, 2:] - T[:, :-2]
    ok = inside.copy()
    ok[[0, -1], :] = False
    ok[:, [0, -1]] = False
    yc = (np.arange(H, dtype=np.int64) - (H >> 1))[:, None] + np.zeros((1, W), np.int64)
    xc = (np.arange(W, dtype=np.int64) - (W >> 1))[None, :] + np.zeros((H, 1), np.int64)
    sd = [v[ok] for v in (gy * yc, gy * xc, gy, gx * yc, gx * xc, gx)]
    e = e[ok]
    k = 0
    for i in range(6):
        for j in range(i, 6):
            out[k] = int((sd[i] * sd[j]).sum())
            k += 1
    for i in range(6):
        out[21 + i] = int((sd[i] * e).sum())
    out[27], out[28] = int((e * e).sum()), int(ok.sum())
    return out


def statement_sums(sources, frames, cands):
    """int64 [n, K, 29]."""
    return np.asarray([[sums(s, f, g) for g in np.asarray(cands)] for s, f in zip(sources, frames)], dtype=np.int64).reshape(len(frames), -1, NSUMS)


def halve(frames):
    """u8 [n, h, w, 3] -> u8 [n, h // 2, w // 2, 3]."""
    f = np.asarray(frames)
    h2, w2 = f.shape[1] // 2, f.shape[2] // 2
    p = f[:, :2 * h2, :2 * w2].astype(np.int64)
    return np.ascontiguousarray(((p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2] + 2) >> 2).astype(np.uint8))


class StatementDecoder:
    """DwtDctSvdDecoder's methods that offmark.resync.register_leak / read_registered_leak drive, over the statement, on host arrays."""

    def align_sums_u8(self, sources, frames, canvas_hw, cands):
        assert tuple(sources.shape[1:3]) == tuple(canvas_hw)
        return statement_sums(sources, frames, cands)

    def halve_u8(self, frames):
        if frames.shape[1] // 2 < 8 or frames.shape[2] // 2 < 8:
            raise ValueError("both halved sides must be at least 8")
        return halve(frames)

    def affine_scores_u8(self, frames, canvas_hw, cands):
        return np.asarray([[af.statement_score(f, canvas_hw, g) for g in np.asarray(cands)] for f in frames], dtype=np.int64)

    def decode_soft_affine_u8(self, frames, canvas_hw, geom, L):
        return np.stack([af.statement_soft(f, canvas_hw, geom, L) for f in frames])
