"""Shared by the DCT codec's resync tests (test_dct_resync_statement.py, test_gpu_dct_resync.py): the NumPy statement of the phase
scores and of the window read-out over the oracle, and the cropped-leak recipe of tests/_resync.py marked with the DCT codec.

Statement: the blocks of phase (py, px) of a frame are the 8x8 blocks of the contiguous crop frame[py:py + 8r, px:px + 8c],
r = (H - py) // 8, c = (W - px) // 8.  The reference's decoder reads that crop as it reads any received frame -- masks and the
luminance mask's frame mean from the crop itself -- and the per-block metric is formed from its debug["c21"] and debug["mask"]
exactly as offmark_oracle.soft_sums forms it: rint(-cos(pi * C21 / (alpha * mask)) * 2^14).  The score of the phase is sum |m|;
the window read-out adds block (i, j) into position (base + i * canvas_cols + j) % L (_resync.canvas_regroup)."""
import functools

import numpy as np

import offmark_oracle as orc
from _resync import H, W, S, F, L8, KEY, COPIES, CHOSEN, CROP, PHASE, BASE      # noqa: F401  (the recipe is _resync's)
from _resync import window, canvas_regroup, recipe_sources, recipe_payloads, recipe_candidates, recipe_segments      # noqa: F401

ALPHA = 20


def block_metric(crop, alpha=ALPHA):
    """int64 [rows * cols], row-major: the per-block soft metric of a frame whose H, W are multiples of 8 (soft_sums' per-block term)."""
    dec = orc.DctDecoderOracle(alpha=alpha)
    dec.decode(orc.bgr2yuv_f32(crop.astype(np.float32)))
    r = dec.debug["c21"].astype(np.float64) / (alpha * dec.debug["mask"])
    return np.rint(-np.cos(np.pi * r) * 16384.0).astype(np.int64).reshape(-1)


def statement_scores(frame, alpha=ALPHA):
    """-> int64 [64]: sum |m| over the blocks of each phase's crop; 0 where the phase has no block."""
    scores = np.zeros(64, np.int64)
    for py in range(8):
        for px in range(8):
            crop, _ = window(frame, py, px)
            if crop is not None:
                scores[8 * py + px] = np.abs(block_metric(crop, alpha)).sum()
    return scores


def statement_window(frame, L, phase, canvas_cols, base=0, alpha=ALPHA):
    crop, (r, c) = window(frame, *phase)
    return canvas_regroup(block_metric(crop, alpha), r, c, canvas_cols, base, L)


def oracle_mark(frame, payload, key=KEY, alpha=ALPHA):
    h, w = frame.shape[:2]
    enc = orc.DctEncoderOracle(alpha=alpha)
    enc.read_wm(orc.shuffle_generate(np.asarray(payload), (1, h * w // 64), key))
    return orc.mark_frame(frame, enc)


def crop_of(frames):
    out = np.ascontiguousarray(frames[:, CROP[0]:, CROP[1]:])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_leak():
    """The recipe marked by the oracle's DCT encoder (alpha 20) and cropped: u8 [12, 61, 83, 3], read-only."""
    src, pay = recipe_sources(), recipe_payloads()
    return crop_of(np.stack([oracle_mark(src[s * F + f], pay[s]) for s in range(S) for f in range(F)]))


@functools.lru_cache(maxsize=None)
def unmarked_leak():
    """The recipe's sources, unmarked, cropped the same way."""
    return crop_of(recipe_sources())


@functools.lru_cache(maxsize=None)
def oracle_leak_scores():
    """statement_scores of every frame of oracle_leak(): int64 [12, 64], read-only."""
    out = np.stack([statement_scores(f) for f in oracle_leak()])
    out.setflags(write=False)
    return out
