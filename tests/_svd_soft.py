"""Shared by the soft read-out tests (test_svd_soft_statement.py, test_gpu_svd_soft.py): the independent NumPy statement of
the DwtDctSvd soft metric (a build extension, not reference semantics) and the noise recipe both modules use.

Statement: the reference's decoder (DwtDctSvdDecoderOracle: Haar LL of channel 1, cv2.dct, float32 LAPACK) gives s0 per unit;
the metric is rint(-sin(2 pi s0 / scale) * 2^14) in float64, summed into position (unit index mod L).  Only the last line
is the extension."""
import functools

import numpy as np

import offmark_oracle as orc

F32 = np.float32
ONE = 16384.0


def statement(frame_u8, L=None, scale=15.0, blk=4):
    """-> dict(s0 float64 [units], m int64 [units], bits (the oracle decoder's, [units]), soft int64 [L] or None)."""
    dec = orc.DwtDctSvdDecoderOracle(scales=(0, scale, 0), blk=blk)
    bits = dec.decode(orc.bgr2yuv_f32(frame_u8.astype(F32))).reshape(-1)
    s0 = dec.debug["s0"].astype(np.float64).reshape(-1)
    m = np.rint(-np.sin(2 * np.pi * s0 / scale) * ONE).astype(np.int64)
    out = dict(s0=s0, m=m, bits=bits[: m.size].astype(np.uint8), soft=None)
    if L is not None:
        out["soft"] = regroup(m, L)
    return out


def regroup(per_unit, L):
    """Per-unit values [units] -> their sums per position [L] (position = unit index mod L)."""
    out = np.zeros(L, np.int64)
    np.add.at(out, np.arange(per_unit.size) % L, per_unit)
    return out


def determined(s0, scale=15.0):
    """tests/test_gpu_svd.py's mask: the residue is more than 1e-3 * max(1, s0 / 100) from a multiple of the step."""
    frac = np.mod(s0, scale)
    return np.minimum(frac, scale - frac) > 1e-3 * np.maximum(1.0, s0 / 100)


def unit_budget(s0, scale=15.0):
    """How far a unit's metric may be from the statement's: two float32 s0 of the same block may differ by
    1e-3 * max(1, s0 / 100) (the project's bound, tests/test_gpu_svd.py:54), the metric's largest slope is 2 pi 2^14 / scale
    per unit of s0, and each side rounds to an integer (+1)."""
    return np.ceil(2 * np.pi * ONE / scale * 1e-3 * np.maximum(1.0, s0 / 100)).astype(np.int64) + 1


def position_budget(s0, L, scale=15.0):
    return regroup(unit_budget(s0, scale), L)


# ---- the noise recipe: 16 segments x 6 frames of 64x96, scale 15, L = 8, key 0, Gaussian noise sigma 6.5 on the marked frames ----
H, W, L8, SEGMENTS, FRAMES, SIGMA = 64, 96, 8, 16, 6, 6.5


def recipe_payload(s):
    return np.array([int(b) for b in format((37 * s + 11) & 255, "08b")], np.uint8)


@functools.lru_cache(maxsize=None)
def noise_recipe():
    """-> dict(noisy u8 [16, 6, H, W, 3], payloads u8 [16, 8], soft int64 [16, 6, 8] and budget int64 [16, 6, 8] (the statement's
    sums and the summed unit budgets), hard u8 [16, 6, 8] (the oracle decoder's per-frame deshuffled payloads))."""
    rng = np.random.default_rng(5)
    noisy = np.empty((SEGMENTS, FRAMES, H, W, 3), np.uint8)
    soft = np.empty((SEGMENTS, FRAMES, L8), np.int64)
    budget = np.empty_like(soft)
    hard = np.empty((SEGMENTS, FRAMES, L8), np.uint8)
    payloads = np.stack([recipe_payload(s) for s in range(SEGMENTS)])
    for s in range(SEGMENTS):
        wm = orc.shuffle_generate(payloads[s], (1, H * W // 64), 0)
        for f in range(FRAMES):
            enc = orc.DwtDctSvdEncoderOracle(scales=(0, 15, 0))
            enc.read_wm(wm)
            marked = orc.mark_frame(orc.synthetic_frame(H, W, 2000 + FRAMES * s + f), enc)
            noisy[s, f] = np.clip(np.rint(marked + rng.normal(0, SIGMA, marked.shape)), 0, 255).astype(np.uint8)
            st = statement(noisy[s, f], L8)
            soft[s, f], budget[s, f] = st["soft"], position_budget(st["s0"], L8)
            hard[s, f] = orc.deshuffle(st["bits"], L8, 0)
    for a in (noisy, soft, budget, hard, payloads):
        a.setflags(write=False)
    return dict(noisy=noisy, payloads=payloads, soft=soft, budget=budget, hard=hard)


def soft_recovered(soft_sums, payloads):
    """Segments whose payload the soft vote recovers: soft_sums [segments, frames, L] added over the frames, un-permuted
    (key 0), read by sign."""
    perm = orc.payload_permutation(L8, 0)
    n = 0
    for s in range(len(payloads)):
        p = np.empty(L8, np.int64)
        p[perm] = np.asarray(soft_sums[s], np.int64).sum(axis=0)
        n += int(np.array_equal((p > 0).astype(np.uint8), payloads[s]))
    return n


def hard_recovered(patterns, payloads):
    """Segments whose payload the reference's vote recovers: the most common whole per-frame pattern [segments, frames, L]."""
    n = 0
    for s in range(len(payloads)):
        v, _ = orc.vote([tuple(int(x) for x in p) for p in patterns[s]])
        n += int(v is not None and np.array_equal(np.asarray(v), payloads[s]))
    return n
