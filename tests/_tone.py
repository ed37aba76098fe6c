"""Shared by the tone tests (test_tone_statement.py, test_gpu_tone.py): the NumPy statement of the three tone calls over
tests/_affine.py's warp, the tone map of the evidence, and a StatementDecoder for offmark.tone.read_toned_leak.

Statement (include/offmark_hip.h: ofmk_histograms_rgb8 / ofmk_tone_sums_rgb8 / ofmk_apply_tone_rgb8), all integers.
Histograms: hist[f, c, v] = the number of pixels of frame f whose channel c equals v.
Tone sums: canvas pixel (y, x) contributes iff the warp's per-pixel ``inside`` holds (no border is left out); with v the warped byte at
(y, x, c), sums[f, k, c, v] += (1, source[f, y, x, c]).  A geometry out of ofmk_affine's range gives zeros.
Apply: out[f, y, x, c] = lut[c, in[f, y, x, c]]."""
import numpy as np

import _affine as af
import _align as al

TONE_MAPS = {"gain-0.85+15": (0.85, 15.0, 1.0), "gain-1.10-8": (1.10, -8.0, 1.0), "gamma-0.85": (1.0, 0.0, 0.85),
             "gamma-1.20": (1.0, 0.0, 1.20), "gain-0.70+40-gamma-1.10": (0.70, 40.0, 1.10)}      # (a, b, gamma): the evidence's five


def tone_map(frames, a, b, gamma):
    """The attack: clip(rint(255 * (clip(a x + b, 0, 255) / 255) ** gamma), 0, 255) on every byte, float64.  u8 -> u8, read-only."""
    x = np.clip(a * np.asarray(frames).astype(np.float64) + b, 0.0, 255.0)
    out = np.ascontiguousarray(np.clip(np.rint(255.0 * (x / 255.0) ** gamma), 0, 255).astype(np.uint8))
    out.setflags(write=False)
    return out


def histograms(frames):
    """u8 [n, h, w, 3] -> int64 [n, 3, 256]."""
    f = np.asarray(frames)
    return np.asarray([[np.bincount(fr[:, :, c].reshape(-1), minlength=256) for c in range(3)] for fr in f], dtype=np.int64).reshape(len(f), 3, 256)


def sums(source, frame, geom):
    """int64 [3, 256, 2] of one source frame (u8 [H, W, 3]) and one leak frame (u8 [h, w, 3]) under one geometry."""
    from offmark import resync
    out = np.zeros((3, 256, 2), np.int64)
    g = tuple(int(v) for v in geom)
    if not resync._affine_ok(g):
        return out
    source = np.asarray(source)
    warped, inside = af.warp(np.asarray(frame), g, source.shape[:2])
    for c in range(3):
        v, s = warped[:, :, c][inside], source[:, :, c][inside].astype(np.int64)
        np.add.at(out[c, :, 0], v, 1)
        np.add.at(out[c, :, 1], v, s)
    return out


def statement_sums(sources, frames, cands):
    """int64 [n, K, 3, 256, 2]."""
    return np.asarray([[sums(s, f, g) for g in np.asarray(cands)] for s, f in zip(sources, frames)], dtype=np.int64).reshape(len(frames), -1, 3, 256, 2)


def apply_tone(frames, lut):
    """u8 [n, h, w, 3], u8 [3, 256] -> u8 [n, h, w, 3]."""
    f, lut = np.asarray(frames), np.asarray(lut, dtype=np.uint8)
    assert lut.shape == (3, 256)
    return np.ascontiguousarray(np.stack([lut[c][f[..., c]] for c in range(3)], axis=-1))


class StatementDecoder(al.StatementDecoder):
    """DwtDctSvdDecoder's methods that offmark.tone.read_toned_leak drives, over the statement, on host arrays."""

    def histograms_u8(self, frames):
        return histograms(frames)

    def tone_sums_u8(self, sources, frames, canvas_hw, cands):
        assert tuple(sources.shape[1:3]) == tuple(canvas_hw)
        return statement_sums(sources, frames, cands)

    def apply_tone_u8(self, frames, lut):
        return apply_tone(frames, lut)
