"""Shared by the planar resync tests (test_planar_resync_statement.py, test_gpu_planar_resync.py): cropped leaks that arrive as
4:2:0 planes, over tests/_resync.py's recipe and the oracle (NumPy only).

The planar recipe: _resync's 3 segments x 4 frames of 72x104 go through the planar chain
    orc.rgb_to_yuv420 -> orc.yuv420_to_rgb -> the oracle encoder of either codec -> orc.rgb_to_yuv420
and the marked PLANES are cropped at CROP = (10, 20): a 62x84 leak at phase (6, 4), base (2 * 13 + 3) % 8 = 5.  A frame's planes
are a tuple (y, u, v) of uint8 arrays; ``pack`` gives the C ABI's bytes in either layout.
Statement: the scores of planes are _resync.statement_scores / _dct_resync.statement_scores of orc.yuv420_to_rgb(planes) with
the odd phases zeroed -- an odd crop offset does not exist on 4:2:0 planes (test_planar_resync_statement.py pins why)."""
import functools

import numpy as np

import offmark_oracle as orc
import _resync as rs
import _dct_resync as dr
import _svd_soft as ss
from _resync import H, W, S, F, L8, KEY, COPIES, CHOSEN      # noqa: F401  (the recipe is _resync's)
from _resync import canvas_regroup, recipe_sources, recipe_payloads, recipe_candidates, recipe_segments      # noqa: F401

ALPHA, SCALE = dr.ALPHA, 15.0
CROP = (10, 20)
PHASE, BASE = (6, 4), 5
LEAK_H, LEAK_W = H - CROP[0], W - CROP[1]          # 62 x 84
ODD_CROP = (11, 21)
CODECS = ("svd", "dct")
EVEN = np.array([py % 2 == 0 and px % 2 == 0 for py in range(8) for px in range(8)])


def to_planes(rgb):
    return orc.rgb_to_yuv420(rgb)


def to_rgb(planes):
    return orc.yuv420_to_rgb(*planes)


def crop_planes(planes, cy, cx, h=None, w=None):
    """The sub-planes for the pixel window [cy : cy + h, cx : cx + w] (to the frame's edge by default); cy, cx, h, w even."""
    y, u, v = planes
    h = y.shape[0] - cy if h is None else h
    w = y.shape[1] - cx if w is None else w
    assert cy % 2 == 0 and cx % 2 == 0 and h % 2 == 0 and w % 2 == 0
    c = (slice(cy // 2, (cy + h) // 2), slice(cx // 2, (cx + w) // 2))
    return tuple(np.ascontiguousarray(a) for a in (y[cy:cy + h, cx:cx + w], u[c], v[c]))


def sub_planes(planes, py, px):
    """sub(py, px): the sub-planes holding the full units of the even phase (py, px), and (rows, cols); None without a unit."""
    Hh, Ww = planes[0].shape
    r, c = (Hh - py) // 8, (Ww - px) // 8
    if r < 1 or c < 1:
        return None, (max(r, 0), max(c, 0))
    return crop_planes(planes, py, px, 8 * r, 8 * c), (r, c)


def pack(frames, layout="i420"):
    """A list of (y, u, v) -> uint8 [n, 1.5 * H * W], the C ABI's bytes."""
    return np.stack([orc.pack_yuv420(*p, layout=layout) for p in frames])


def planar_mark(frame, payload, codec):
    rgb = to_rgb(to_planes(frame))
    marked = rs.oracle_mark(rgb, payload, KEY) if codec == "svd" else dr.oracle_mark(rgb, payload)
    return to_planes(marked)


@functools.lru_cache(maxsize=None)
def marked_planes(codec):
    """The recipe through the planar chain: 12 x (y 72x104, u, v)."""
    src, pay = recipe_sources(), recipe_payloads()
    return tuple(planar_mark(src[s * F + f], pay[s], codec) for s in range(S) for f in range(F))


@functools.lru_cache(maxsize=None)
def oracle_leak(codec):
    """The marked planes cropped at CROP: 12 x (y 62x84, u 31x42, v 31x42)."""
    return tuple(crop_planes(p, *CROP) for p in marked_planes(codec))


@functools.lru_cache(maxsize=None)
def unmarked_leak():
    """The recipe's sources as planes, unmarked, cropped the same way."""
    return tuple(crop_planes(to_planes(f), *CROP) for f in recipe_sources())


@functools.lru_cache(maxsize=None)
def odd_leak(codec):
    """What an odd crop offset has to be on planes: convert, crop at ODD_CROP, trim to even sizes (60x82), convert back."""
    out = []
    for p in marked_planes(codec):
        rgb = to_rgb(p)[ODD_CROP[0]:, ODD_CROP[1]:]
        out.append(to_planes(np.ascontiguousarray(rgb[:rgb.shape[0] // 2 * 2, :rgb.shape[1] // 2 * 2])))
    return tuple(out)


def unit_metric(rgb, codec):
    """-> (m int64 [units], budget int64 [units]): the codec's per-unit soft metric of an RGB frame with H, W multiples of 8, and
    how far a device metric may be from it.  DwtDctSvd: _svd_soft.unit_budget.  DCT: tests/test_gpu_dct_resync.py holds its
    kernels against the device read-out only and sets no budget against the statement, so this is the project's one bound on
    the DCT soft metric against the oracle, tests/test_gpu_parity.py's 3 fixed-point units per block (C21 / step within ~1e-6
    relative); measured on the recipe leak: at most 1 per PHASE, against a budget of 210."""
    if codec == "svd":
        st = ss.statement(rgb, scale=SCALE)
        return st["m"], ss.unit_budget(st["s0"], SCALE)
    m = dr.block_metric(rgb, ALPHA)
    return m, np.full(m.size, 3, np.int64)


def statement_scores(planes, codec):
    """-> (scores int64 [64], budget int64 [64]): _resync.statement_scores / _dct_resync.statement_scores of to_rgb(planes) with
    the odd phases zeroed, computed for the 16 even phases only (the same per-phase terms: the metric of the phase's crop)."""
    rgb = to_rgb(planes)
    scores, budget = np.zeros(64, np.int64), np.zeros(64, np.int64)
    for py in range(0, 8, 2):
        for px in range(0, 8, 2):
            crop, _ = rs.window(rgb, py, px)
            if crop is not None:
                m, b = unit_metric(crop, codec)
                scores[8 * py + px], budget[8 * py + px] = np.abs(m).sum(), b.sum()
    return scores, budget


@functools.lru_cache(maxsize=None)
def leak_scores(codec, which="marked"):
    """statement_scores of every frame of oracle_leak(codec) / unmarked_leak() / odd_leak(codec): int64 [12, 64], read-only."""
    frames = {"marked": lambda: oracle_leak(codec), "unmarked": unmarked_leak, "odd": lambda: odd_leak(codec)}[which]()
    out = np.stack([statement_scores(p, codec)[0] for p in frames])
    out.setflags(write=False)
    return out


def statement_window(planes, codec, L, phase, canvas_cols, base=0):
    sub, (r, c) = sub_planes(planes, *phase)
    return canvas_regroup(unit_metric(to_rgb(sub), codec)[0], r, c, canvas_cols, base, L)
