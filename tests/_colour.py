"""Shared by the colour tests (test_colour_statement.py, test_gpu_colour.py): the NumPy statement of the two colour calls over
tests/_affine.py's warp, the colour attacks of the evidence, and a StatementDecoder for offmark.colour.read_coloured_leak.

Statement (include/offmark_hip.h: ofmk_colour_sums_rgb8 / ofmk_apply_colour_rgb8), all integers.
Colour sums: canvas pixel (y, x) contributes iff the warp's per-pixel ``inside`` holds (no border is left out) AND all three warped
leak bytes are in 1..254 (a clipped pixel says nothing about the matrix).  With l the three warped bytes and s the three source bytes at
(y, x): [0] the count, [1..3] sum l_c, [4..6] sum s_c, [7..12] sum l_i l_j for (i, j) = (0,0), (0,1), (0,2), (1,1), (1,2), (2,2),
[13..18] sum s_i s_j in the same order, [19 + 3 i + j] sum l_i s_j.  A geometry out of ofmk_affine's range gives 28 zeros.
Apply: m is int32 [3][4] in Q16, row c the three coefficients and then the offset;
out[c] = clip((m[c][0] in[0] + m[c][1] in[1] + m[c][2] in[2] + m[c][3] + 32768) >> 16, 0, 255), an arithmetic shift; legal
|coefficient| <= 2^21 and |offset| <= 2^28, so the sum stays inside int32."""
import numpy as np

import _affine as af
import _tone as tn

NSUMS = 28
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
MAX_COEFF, MAX_OFFSET = 1 << 21, 1 << 28
IDENTITY_MATRIX = np.asarray([[65536, 0, 0, 0], [0, 65536, 0, 0], [0, 0, 65536, 0]], np.int32)

# ---- the attacks: clip(rint(a * (M x) + b), 0, 255) on every pixel, the channels in stored order ----------------------------------
W601, W709 = (0.299, 0.587, 0.114), (0.2126, 0.7152, 0.0722)


def ycbcr(w):
    """A(w): the full-range RGB -> YCbCr matrix of the luma weights w (the 128 offsets of Cb, Cr cancel in every product below)."""
    wr, wg, wb = w
    y = np.asarray([wr, wg, wb], np.float64)
    return np.stack([y, (np.asarray([0.0, 0.0, 1.0]) - y) / (2.0 * (1.0 - wb)), (np.asarray([1.0, 0.0, 0.0]) - y) / (2.0 * (1.0 - wr))])


def sat(s):
    return s * np.eye(3) + (1.0 - s) * np.outer(np.ones(3), np.asarray(W601))


def hue(deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    a = ycbcr(W601)
    return np.linalg.inv(a) @ np.asarray([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]]) @ a


M_601_AS_709 = np.linalg.inv(ycbcr(W709)) @ ycbcr(W601)
M_709_AS_601 = np.linalg.inv(ycbcr(W601)) @ ycbcr(W709)

ATTACKS = {"identity": (np.eye(3), 1.0, 0.0), "sat-0.8": (sat(0.8), 1.0, 0.0), "sat-1.25": (sat(1.25), 1.0, 0.0), "sat-0.6": (sat(0.6), 1.0, 0.0),
           "hue+10": (hue(10.0), 1.0, 0.0), "hue-20": (hue(-20.0), 1.0, 0.0), "601as709": (M_601_AS_709, 1.0, 0.0),
           "709as601": (M_709_AS_601, 1.0, 0.0), "sat-0.8-gain-0.85+15": (sat(0.8), 0.85, 15.0),
           "hue+10-sat-1.2-gain-1.10-8": (hue(10.0) @ sat(1.2), 1.10, -8.0)}      # (M, a, b): the evidence's ten


def colour_map(frames, M, a=1.0, b=0.0):
    """The attack: clip(rint(a * (M x) + b), 0, 255) on every pixel, float64.  u8 -> u8, read-only."""
    x = np.asarray(frames).astype(np.float64) @ np.asarray(M, np.float64).T
    out = np.ascontiguousarray(np.clip(np.rint(a * x + b), 0, 255).astype(np.uint8))
    out.setflags(write=False)
    return out


# ---- the statements ------------------------------------------------------------------------------------------------------------------
def sums(source, frame, geom):
    """int64 [28] of one source frame (u8 [H, W, 3]) and one leak frame (u8 [h, w, 3]) under one geometry."""
    from offmark import resync
    out = np.zeros(NSUMS, np.int64)
    g = tuple(int(v) for v in geom)
    if not resync._affine_ok(g):
        return out
    source = np.asarray(source)
    warped, inside = af.warp(np.asarray(frame), g, source.shape[:2])
    ok = inside & ((warped >= 1) & (warped <= 254)).all(axis=2)
    l, s = warped[ok].astype(np.int64), source[ok].astype(np.int64)      # [pixels, 3]
    out[0] = len(l)
    out[1:4], out[4:7] = l.sum(axis=0), s.sum(axis=0)
    for n, (i, j) in enumerate(PAIRS):
        out[7 + n], out[13 + n] = (l[:, i] * l[:, j]).sum(), (s[:, i] * s[:, j]).sum()
    for i in range(3):
        for j in range(3):
            out[19 + 3 * i + j] = (l[:, i] * s[:, j]).sum()
    return out


def statement_sums(sources, frames, cands):
    """int64 [n, K, 28]."""
    return np.asarray([[sums(s, f, g) for g in np.asarray(cands)] for s, f in zip(sources, frames)], dtype=np.int64).reshape(len(frames), -1, NSUMS)


def legal(matrix) -> bool:
    m = np.asarray(matrix, dtype=np.int64)
    return m.shape == (3, 4) and bool((np.abs(m[:, :3]) <= MAX_COEFF).all() and (np.abs(m[:, 3]) <= MAX_OFFSET).all())


def apply_colour(frames, matrix):
    """u8 [n, h, w, 3], int32 [3, 4] in Q16 -> u8 [n, h, w, 3]; int32 throughout, as the device."""
    f, m = np.asarray(frames), np.asarray(matrix)
    assert legal(m) and m.dtype.kind == "i"
    m = m.astype(np.int32)
    x = f.astype(np.int32)
    acc = [m[c, 0] * x[..., 0] + m[c, 1] * x[..., 1] + m[c, 2] * x[..., 2] + m[c, 3] + np.int32(32768) for c in range(3)]
    assert all(a.dtype == np.int32 for a in acc)
    return np.ascontiguousarray(np.stack([np.clip(a >> 16, 0, 255) for a in acc], axis=-1).astype(np.uint8))


class StatementDecoder(tn.StatementDecoder):
    """DwtDctSvdDecoder's methods that offmark.colour.read_coloured_leak drives, over the statement, on host arrays."""

    def colour_sums_u8(self, sources, frames, canvas_hw, cands):
        assert tuple(sources.shape[1:3]) == tuple(canvas_hw)
        return statement_sums(sources, frames, cands)

    def apply_colour_u8(self, frames, matrix):
        return apply_colour(frames, matrix)
