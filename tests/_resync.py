"""Shared by the resync tests (test_resync_statement.py, test_gpu_resync.py): the NumPy statement of the phase scores and of the
window read-out over tests/_svd_soft.py's statement of the unit metric, and the cropped-leak recipe both modules use.

Statement: the units of phase (py, px) of a frame are the 8x8 blocks of frame[py:py + 8r, px:px + 8c], r = (H - py) // 8,
c = (W - px) // 8; the reference's decoder on that crop gives their s0, _svd_soft.statement their metric m.  The score of the
phase is sum |m|; the window read-out adds unit (i, j) into position (base + i * canvas_cols + j) % L."""
import functools

import numpy as np

import offmark_oracle as orc
import _svd_soft as ss


def window(frame, py, px):
    """The contiguous crop that holds the full units of phase (py, px), and its (rows, cols) in units; None without a unit."""
    H, W = frame.shape[:2]
    r, c = (H - py) // 8, (W - px) // 8
    if r < 1 or c < 1:
        return None, (max(r, 0), max(c, 0))
    return np.ascontiguousarray(frame[py:py + 8 * r, px:px + 8 * c]), (r, c)


def statement_scores(frame, scale=15.0):
    """-> (scores int64 [64], budget int64 [64]): sum |m| per phase, and the summed _svd_soft.unit_budget of the phase's units."""
    scores, budget = np.zeros(64, np.int64), np.zeros(64, np.int64)
    for py in range(8):
        for px in range(8):
            crop, _ = window(frame, py, px)
            if crop is None:
                continue
            st = ss.statement(crop, scale=scale)
            scores[8 * py + px] = np.abs(st["m"]).sum()
            budget[8 * py + px] = ss.unit_budget(st["s0"], scale).sum()
    return scores, budget


def canvas_regroup(per_unit, rows, cols, canvas_cols, base, L):
    """Per-unit values [rows * cols] (row-major) -> sums per position (base + i * canvas_cols + j) % L, int64 [L]."""
    i, j = np.divmod(np.arange(rows * cols), cols)
    out = np.zeros(L, np.int64)
    np.add.at(out, (base + i * canvas_cols + j) % L, np.asarray(per_unit, np.int64))
    return out


def statement_window(frame, L, phase, canvas_cols, base=0, scale=15.0):
    crop, (r, c) = window(frame, *phase)
    return canvas_regroup(ss.statement(crop, scale=scale)["m"], r, c, canvas_cols, base, L)


def oracle_mark(frame, payload, key=0, scale=15):
    H, W = frame.shape[:2]
    enc = orc.DwtDctSvdEncoderOracle(scales=(0, scale, 0))
    enc.read_wm(orc.shuffle_generate(np.asarray(payload), (1, H * W // 64), key))
    return orc.mark_frame(frame, enc)


# ---- the cropped-leak recipe: 3 segments x 4 frames of 72x104, seeds 3000 + 4 s + f, payloads payload_for_segment(s + 1, chosen[s]),
# 2 copies, key 0, scale 15; the leak is marked[:, 11:72, 21:104] (61x83): phase (5, 3), base (2 * 13 + 3) % 8 = 5 ----
H, W, S, F, L8, KEY, COPIES = 72, 104, 3, 4, 8, 0, 2
CHOSEN = (1, 0, 1)
CROP = (11, 21)
PHASE, BASE = (5, 3), 5


def recipe_sources():
    return np.stack([orc.synthetic_frame(H, W, 3000 + 4 * s + f) for s in range(S) for f in range(F)])


def recipe_payloads():
    from offmark.fingerprint import payload_for_segment
    return [payload_for_segment(s + 1, CHOSEN[s]) for s in range(S)]


def recipe_candidates():
    from offmark.fingerprint import payload_for_segment
    return [[payload_for_segment(s + 1, c) for c in range(COPIES)] for s in range(S)]


def recipe_segments():
    return np.repeat(np.arange(S), F)


@functools.lru_cache(maxsize=None)
def oracle_leak():
    """The recipe marked by the oracle encoder and cropped: u8 [12, 61, 83, 3], read-only."""
    src, pay = recipe_sources(), recipe_payloads()
    marked = np.stack([oracle_mark(src[s * F + f], pay[s], KEY) for s in range(S) for f in range(F)])
    leak = np.ascontiguousarray(marked[:, CROP[0]:, CROP[1]:])
    leak.setflags(write=False)
    return leak
