"""Shared by the mask-leaf tests (test_mask_leaves_statement.py, test_kernel_arithmetic.py, test_gpu_mask_leaves.py,
test_gpu_parity.py): the DCT codec's two perceptual masks as trees with NAMED leaves, a seeded pool of 8x8 blocks that reaches
every feasible leaf and both sides of every threshold, the decidability margin tau, and two small frames ("the zoo") assembled
from the pool.  Everything is stated on oracle/offmark_oracle.py (texture_features, texture_from_features, luminance_from_dc,
DctEncoderOracle, DctDecoderOracle); nothing here reads the kernels.

Texture tree (texture_from_features / dct_encoder.py:70-102), features a00 = |A00|, dcl, eh, e; h = eh - e, l = dcl - a00,
l_e = l / e, lpe = l + e, le_h = lpe / h, eph = e + h:

    eh <= 125 ............................................. inactive                       1
    eh  > 900 ("big", constants a, b = 1.4, 1.1):
        cond: first  = l_e >= a and le_h >= b             big_first_1125 / big_first_125     1.125 if lpe <= 400 else 1.25
              second = l_e >= b and le_h >= a (only)      big_second_1125 / big_second_125
              gt4    = le_h > 4 (only)                    big_gt4_1125 / big_gt4_125
        else ............................................. big_ramp                       1 + 1.25 (eh - 290) / 1510
    125 < eh <= 900 ("small", a, b = 2.3, 1.6):
        cond as above .................................... small_first_1125 ... small_gt4_125
        else eph > 290 ................................... small_ramp
        else ............................................. small_one                      1

The three big_*_1125 leaves cannot occur.  With l >= 0 (dcl is a00 plus five absolute values), cond in the big arm means
le_h = (l + e) / h >= 1.1 (first clause: b; second clause: a = 1.4; third: > 4), so h <= (l + e) / 1.1 and
900 < e + h <= e + (l + e) / 1.1 <= (l + e) (1 + 1 / 1.1) = 1.909 (l + e), i.e. l + e > 471 > 400: the step is always 1.25.
(h <= 0 makes le_h negative, infinite or nan and cond false unless l_e and le_h pass, which needs le_h >= 1.1 again.)
pool() asserts that no block lands there.

Non-finite ratios (e == 0 or h == 0) do not occur on an active block (eh > 125) of the pool, which pool() asserts: rounding to
u8 leaves energy in all three coefficient groups.  They are covered by the float32 replay of texture_code() on hand-built
feature tuples only (test_kernel_arithmetic.py).

Luminance tree (luminance_from_dc / dct_encoder.py:41-67), m = A00 / 8, mean = max(90, frame mean of m):
    m > mean: above (a ramp);  m < 15: lt15 (1.25);  m < 25: lt25 (1.125);  else one (1) -- each under a clamped
    (frame mean <= 90) and an unclamped frame mean, which is a property of the frame: the zoo has one frame of each kind.

tau, the decidability margin: 10 x the largest absolute difference, over the pool, between the oracle's float32 features
(a00, dcl, eh, e) and the same sums formed in float64 from a float64 DCT of the same float32 Y block -- ten times the
oracle's own level, the project's habit (tests/_svd_repeated.py).  A block is TAU-STABLE when the tree's leaf is the same at
all 81 perturbations of the four features by {-tau, 0, +tau}; for luminance m and the frame mean are perturbed by tau / 8
(a00 is 8 m).  The ADMITTED SET of an unstable block is the set of values over those perturbations (plus the oracle's own);
ramp values are admitted within 1.25 tau / 1510 + 2e-6 (texture) and 2 (tau / 8) / 165 + 2e-6 (luminance)."""
import functools
import itertools
import math
from collections import namedtuple

import numpy as np

import offmark_oracle as orc

F32, F64 = np.float32, np.float64

PARAMS = dict(A1=2.3, B1=1.6, A2=1.4, B2=1.1, ACT=125.0, BIG=900.0, LPE=400.0, EPH=290.0, GT4=4.0)

TEX_LEAVES = ("inactive",
              "big_first_1125", "big_first_125", "big_second_1125", "big_second_125", "big_gt4_1125", "big_gt4_125", "big_ramp",
              "small_first_1125", "small_first_125", "small_second_1125", "small_second_125", "small_gt4_1125", "small_gt4_125",
              "small_ramp", "small_one")
TEX_INFEASIBLE = ("big_first_1125", "big_second_1125", "big_gt4_1125")
TEX_FEASIBLE = tuple(n for n in TEX_LEAVES if n not in TEX_INFEASIBLE)
T_INACTIVE, T_BIG_RAMP, T_SMALL_RAMP, T_SMALL_ONE = 0, 7, 14, 15
# the 13 comparisons: (name, quantity, parameter).  ">=" for the ratio constants, ">" for the others, as the reference writes them
COMPARISONS = (("eh>125", "eh", "ACT"), ("eh>900", "eh", "BIG"), ("lpe>400", "lpe", "LPE"), ("eph>290", "eph", "EPH"),
               ("le_h>4", "le_h", "GT4"),
               ("l_e>=2.3", "l_e", "A1"), ("le_h>=1.6", "le_h", "B1"), ("l_e>=1.6", "l_e", "B1"), ("le_h>=2.3", "le_h", "A1"),
               ("l_e>=1.4", "l_e", "A2"), ("le_h>=1.1", "le_h", "B2"), ("l_e>=1.1", "l_e", "B2"), ("le_h>=1.4", "le_h", "A2"))
LUM_LEAVES = ("above", "lt15", "lt25", "one")
NEAR = 1e-3                    # "near a threshold": within 1e-3 relative
MIN_LEAF, MIN_SIDE = 8, 4      # tau-stable zoo blocks per leaf / per side of a comparison
C21_FLOOR = 1.0                # every pool block's |C21| is far above the sign tolerance 1e-3


def budget(n, frac, floor=1):
    return max(floor, int(np.floor(n * frac)))


def write_report(name, lines):
    """Print a table of a test and, with OFFMARK_MASK_LEAVES_OUT=<directory> set, also write it there as ``name`` (the
    committed copy of these tables is profiles/mask_leaves_tests.txt)."""
    import os
    print("\n".join(lines))
    out = os.environ.get("OFFMARK_MASK_LEAVES_OUT")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, name), "w") as f:
            f.write("\n".join(lines) + "\n")


# ------------------------------------------------------------------------------------------------------------------------
# the trees
# ------------------------------------------------------------------------------------------------------------------------
def tex_quantities(a00, dcl, eh, e):
    """The tree's quantities in the inputs' own precision: float32 inputs give the reference's float32 scalars."""
    with np.errstate(divide="ignore", invalid="ignore"):
        h = eh - e
        l = dcl - a00
        lpe = l + e
        return dict(eh=eh, lpe=lpe, eph=e + h, l_e=l / e, le_h=lpe / h)


def tex_compare(q, params=PARAMS):
    """[13, ...] bool.  Every comparison in float64 (numpy 1.23 promotion; exact for the integer thresholds)."""
    with np.errstate(invalid="ignore"):
        return np.stack([(np.asarray(q[name]).astype(F64) >= params[p]) if ">=" in label else (np.asarray(q[name]).astype(F64) > params[p])
                         for label, name, p in COMPARISONS])


def tex_leaf_of(c):
    """Leaf index (TEX_LEAVES) from the 13 comparison outcomes."""
    active, big, step125, eph, gt4 = c[0], c[1], c[2], c[3], c[4]
    leaf = np.zeros(c.shape[1:], np.int8)
    for arm, base, k in ((big, 1, 9), (~big, 8, 5)):
        first, second = c[k] & c[k + 1], c[k + 2] & c[k + 3]
        clause = np.where(first, 0, np.where(second, 1, np.where(gt4, 2, 3)))
        inner = np.where(clause < 3, base + 2 * clause + step125,
                         T_BIG_RAMP if base == 1 else np.where(eph, T_SMALL_RAMP, T_SMALL_ONE))
        leaf = np.where(active & arm, inner, leaf)
    return leaf.astype(np.int8)


def ramp_value(eh):
    return 1 + 1.25 * (np.asarray(eh).astype(F64) - 290) / (1800 - 290)


def tex_value_of(leaf, eh):
    leaf = np.asarray(leaf).astype(np.int64)
    step = ((leaf >= 1) & (leaf <= 6)) | ((leaf >= 8) & (leaf <= 13))
    v125 = np.where(leaf >= 8, (leaf - 8) % 2 == 1, (leaf - 1) % 2 == 1)          # within an arm: ..._1125 then ..._125
    out = np.where(step, np.where(v125, 1.25, 1.125), 1.0)
    return np.where((leaf == T_BIG_RAMP) | (leaf == T_SMALL_RAMP), ramp_value(eh), out)


TexLabel = namedtuple("TexLabel", "leaf value cmp rel decisive")


def tex_label(a00, dcl, eh, e, params=PARAMS, want_decisive=True):
    """-> TexLabel: leaf index, value (float64), the 13 outcomes, each comparison's relative distance (quantity - threshold) /
    threshold, and per comparison whether it is DECISIVE for the block: flipping that outcome alone changes the value."""
    q = tex_quantities(a00, dcl, eh, e)
    c = tex_compare(q, params)
    leaf = tex_leaf_of(c)
    value = tex_value_of(leaf, eh)
    rel = np.stack([(np.asarray(q[name]).astype(F64) - params[p]) / params[p] for _, name, p in COMPARISONS])
    dec = None
    if want_decisive:
        dec = np.zeros(c.shape, bool)
        for k in range(len(COMPARISONS)):
            c2 = c.copy()
            c2[k] = ~c2[k]
            dec[k] = tex_value_of(tex_leaf_of(c2), eh) != value
    return TexLabel(leaf, value, c, rel, dec)


def lum_label(m, frame_mean):
    """-> (leaf index (LUM_LEAVES), value float64) for block means m under the frame's raw mean (clamped at 90 here)."""
    m = np.asarray(m, F64)
    mean = np.maximum(orc.L_MIN, np.asarray(frame_mean, F64))
    f_ref = 1 + (mean - orc.L_MIN) * (orc.F_MAX - 1) / (orc.L_MAX - orc.L_MIN)
    hi = m > mean
    with np.errstate(divide="ignore", invalid="ignore"):
        ramp = 1 + (m - mean) / (orc.L_MAX - mean) * (orc.F_MAX - f_ref)
    leaf = np.where(hi, 0, np.where(m < 15, 1, np.where(m < 25, 2, 3))).astype(np.int8)
    return leaf, np.where(hi, ramp, np.where(m < 15, 1.25, np.where(m < 25, 1.125, 1.0)))


# ------------------------------------------------------------------------------------------------------------------------
# tau-stability and admitted sets
# ------------------------------------------------------------------------------------------------------------------------
Stability = namedtuple("Stability", "stable admitted")      # admitted: {flat block index: sorted list of values} for the unstable blocks


def tex_ramp_slack(tau):
    return 1.25 * tau / 1510 + 2e-6


def lum_ramp_slack(tau):
    return 2 * (tau / 8) / 165 + 2e-6


def tex_stability(a00, dcl, eh, e, tau, params=PARAMS):
    f = [np.asarray(x, F32).astype(F64).reshape(-1) for x in (a00, dcl, eh, e)]
    base = tex_label(*[np.asarray(x, F32).reshape(-1) for x in (a00, dcl, eh, e)], params=params, want_decisive=False)
    stable = np.ones(f[0].shape, bool)
    offs = list(itertools.product((-tau, 0.0, tau), repeat=4))
    for d in offs:
        stable &= tex_leaf_of(tex_compare(tex_quantities(*[x + dd for x, dd in zip(f, d)]), params)) == base.leaf
    idx = np.nonzero(~stable)[0]
    admitted = {}
    if idx.size:
        vals = np.stack([tex_label(*[x[idx] + dd for x, dd in zip(f, d)], params=params, want_decisive=False).value for d in offs]
                        + [base.value[idx]])
        for j, i in enumerate(idx):
            admitted[int(i)] = sorted(set(float(v) for v in vals[:, j]))
    return Stability(stable, admitted)


def lum_stability(m, frame_mean, tau):
    m = np.asarray(m, F64).reshape(-1)
    t = tau / 8
    leaf0, val0 = lum_label(m, frame_mean)
    stable = np.ones(m.shape, bool)
    offs = list(itertools.product((-t, 0.0, t), repeat=2))
    for dm, dmean in offs:
        stable &= lum_label(m + dm, frame_mean + dmean)[0] == leaf0
    idx = np.nonzero(~stable)[0]
    admitted = {}
    if idx.size:
        vals = np.stack([lum_label(m[idx] + dm, frame_mean + dmean)[1] for dm, dmean in offs] + [val0[idx]])
        for j, i in enumerate(idx):
            admitted[int(i)] = sorted(set(float(v) for v in vals[:, j]))
    return Stability(stable, admitted)


def in_admitted(value, admitted, slack):
    return any(abs(value - v) <= slack for v in admitted)


def nearest_admitted(value, admitted):
    return min(admitted, key=lambda v: abs(v - value))


# ------------------------------------------------------------------------------------------------------------------------
# features of u8 RGB blocks, as the oracle forms them and in float64
# ------------------------------------------------------------------------------------------------------------------------
def _dct64(y):
    t = orc._dct1d_last(np.asarray(y, F64))
    return np.swapaxes(orc._dct1d_last(np.swapaxes(t, -1, -2)), -1, -2)


_E_TERMS = ((3, 0), (4, 0), (5, 0), (6, 0), (0, 3), (0, 4), (0, 5), (0, 6), (2, 1), (1, 2), (2, 2), (3, 3))
_L_TERMS = ((0, 1), (0, 2), (1, 0), (1, 1), (2, 0))
_H_TERMS = tuple((p, q) for p in range(8) for q in range(8) if (p, q) != (0, 0) and (p, q) not in _E_TERMS and (p, q) not in _L_TERMS)

Features = namedtuple("Features", "a00 dcl eh e ydc c21 f64")       # f64 = (a00, dcl, eh, e) in float64 from a float64 DCT


def features_of_y(y):
    """y: (..., 8, 8) float32 Y blocks -> Features without c21."""
    y = np.asarray(y, F32)
    coef = orc.dct8x8(y)
    a = np.abs(coef)
    dcl, eh, e = orc.texture_features(a)
    a64 = np.abs(_dct64(y.astype(F64)))
    dcl64 = a64[..., 0, 0] + sum(a64[..., p, q] for p, q in _L_TERMS)
    f64 = (a64[..., 0, 0], dcl64, a64.sum((-1, -2)) - dcl64, sum(a64[..., p, q] for p, q in _E_TERMS))
    return Features(a[..., 0, 0], dcl, eh, e, coef[..., 0, 0], None, f64)


def features_of_blocks(rgb):
    """rgb: (..., 8, 8, 3) uint8 blocks."""
    yuv = orc.bgr2yuv_f32(np.asarray(rgb).astype(F32))
    ft = features_of_y(yuv[..., 0])
    return ft._replace(c21=orc.dct8x8(yuv[..., 1])[..., 2, 1])


def features_of_frame(frame):
    """frame: u8 [H, W, 3] -> Features per block [rows, cols] (what DctEncoderOracle / DctDecoderOracle see)."""
    yuv = orc.bgr2yuv_f32(frame.astype(F32))
    ft = features_of_y(orc.to_blocks(yuv[:, :, 0]))
    return ft._replace(c21=orc.dct8x8(orc.to_blocks(yuv[:, :, 1]))[..., 2, 1])


def feature_level(ft):
    """Largest |float32 feature - float64 feature| over the blocks: the oracle's own level."""
    return max(float(np.abs(np.asarray(a).astype(F64) - b).max()) for a, b in zip((ft.a00, ft.dcl, ft.eh, ft.e), ft.f64))


# ------------------------------------------------------------------------------------------------------------------------
# the seeded pool
# ------------------------------------------------------------------------------------------------------------------------
def chroma_pattern(amp=8):
    """Integer (2,1)-shaped pattern for channel 0: antisymmetric in x, so it sums to zero and leaves the block mean alone."""
    r, x = np.mgrid[0:8, 0:8]
    return np.around(amp * np.cos((2 * r + 1) * 2 * np.pi / 16) * np.cos((2 * x + 1) * np.pi / 16)).astype(np.int16)


def _blocks_from_amplitudes(rng, amp_l, amp_e, amp_h, even):
    """u8 RGB blocks from DCT-domain group amplitudes (the summed |coefficient| of the five dcl terms, the twelve e terms and
    the other 46): random split and signs inside each group, a random DC, inverse transform, round, clip; two constant colour
    offsets and the (2,1) chroma pattern on channel 0."""
    n = amp_l.size
    coef = np.zeros((n, 8, 8), F32)
    for terms, amp in ((_L_TERMS, amp_l), (_E_TERMS, amp_e), (_H_TERMS, amp_h)):
        w = rng.random((n, len(terms)))
        w = np.where(even[:, None], 0.5 + w, w ** 2)
        w = w / w.sum(1, keepdims=True) * amp[:, None] * rng.choice((-1.0, 1.0), (n, len(terms)))
        for k, (p, q) in enumerate(terms):
            coef[:, p, q] = w[:, k]
    coef[:, 0, 0] = 8 * rng.uniform(8, 247, n)
    gray = np.around(np.clip(orc.idct8x8(coef), 0, 255)).astype(np.int16)
    rgb = np.repeat(gray[..., None], 3, axis=-1)
    rgb[..., 0] += rng.integers(-12, 13, (n, 1, 1)) + chroma_pattern()[None]
    rgb[..., 2] += rng.integers(-12, 13, (n, 1, 1))
    return np.clip(rgb, 0, 255).astype(np.uint8)


def _loguniform(rng, lo, hi, n):
    return np.exp(rng.uniform(math.log(lo), math.log(hi), n))


def _biased_amplitudes(rng, n, eh_lo, eh_hi, ca, cb):
    """Group amplitudes aimed at the neighbourhood of an arm's ratio constants: eh log-uniform over the arm, l_e and le_h
    uniform over [0.8 cb, 1.2 ca]."""
    eh = _loguniform(rng, eh_lo, eh_hi, n)
    l_e, le_h = rng.uniform(0.8 * cb, 1.2 * ca, n), rng.uniform(0.8 * cb, 1.2 * ca, n)
    e = eh / (1 + (1 + l_e) / le_h)
    return l_e * e, e, eh - e


Pool = namedtuple("Pool", "rgb ft label stab tau level")

POOL_SEED, POOL_UNBIASED, POOL_BIASED = 20261, 100_000, 30_000


def _label(ft):
    return tex_label(ft.a00, ft.dcl, ft.eh, ft.e)


@functools.lru_cache(maxsize=None)
def pool():
    """The seeded pool: POOL_UNBIASED blocks with the three group amplitudes log-uniform over 1 .. 1200, POOL_BIASED blocks aimed
    at each arm's ratio constants (the unbiased draw leaves single digits near the big arm's), then +-1 LSB resampling around
    the nearest misses of every threshold side that still lacks blocks.  tau is measured on the whole pool."""
    rng = np.random.default_rng(POOL_SEED)
    n = POOL_UNBIASED
    parts = [_blocks_from_amplitudes(rng, *(_loguniform(rng, 1, 1200, n) for _ in range(3)), np.zeros(n, bool))]
    for lo, hi, ca, cb in ((900, 2200, PARAMS["A2"], PARAMS["B2"]), (125, 900, PARAMS["A1"], PARAMS["B1"])):
        parts.append(_blocks_from_amplitudes(rng, *_biased_amplitudes(rng, POOL_BIASED // 2, lo, hi, ca, cb), np.ones(POOL_BIASED // 2, bool)))
    rgb = np.concatenate(parts)
    ft = features_of_blocks(rgb)
    keep = np.abs(ft.c21) >= C21_FLOOR            # clipping at 0 / 255 can flatten the chroma pattern: those blocks are dropped
    rgb, ft = rgb[keep], features_of_blocks(rgb[keep])
    lab = _label(ft)
    # +-1 LSB resampling around near misses: for each (comparison, side) short of blocks, the decisive blocks nearest the threshold
    extra = []
    for k in range(len(COMPARISONS)):
        for side in (False, True):
            near = lab.decisive[k] & (lab.cmp[k] == side) & (np.abs(lab.rel[k]) <= NEAR)
            if near.sum() >= 3 * MIN_SIDE:
                continue
            cand = np.nonzero(lab.decisive[k] & (np.abs(lab.rel[k]) <= 0.03))[0]
            cand = cand[np.argsort(np.abs(lab.rel[k][cand]))][:60]
            reps = np.repeat(rgb[cand], 20, axis=0).astype(np.int16)
            m = reps.shape[0]
            for _ in range(3):          # three pixels, all channels: Y moves by one level there
                reps[np.arange(m), rng.integers(0, 8, m), rng.integers(0, 8, m)] += rng.choice((-1, 1), (m, 1))
            extra.append(np.clip(reps, 0, 255).astype(np.uint8))
    if extra:
        rgb = np.concatenate([rgb] + extra)
        ft = features_of_blocks(rgb)
        keep = np.abs(ft.c21) >= C21_FLOOR
        rgb, ft = rgb[keep], features_of_blocks(rgb[keep])
        lab = _label(ft)
    assert not np.isin(lab.leaf, [TEX_LEAVES.index(nm) for nm in TEX_INFEASIBLE]).any(), "a block on an infeasible leaf: the argument in the module text is wrong"
    assert np.abs(ft.c21).min() >= C21_FLOOR, "a sign-ambiguous pool block"
    assert np.isfinite(lab.rel[:, lab.cmp[0]]).all(), "a non-finite ratio on an active block: the module text says there is none"
    level = feature_level(ft)
    tau = 10 * level
    stab = tex_stability(ft.a00, ft.dcl, ft.eh, ft.e, tau)
    for a in (rgb,) + tuple(ft[:6]) + tuple(ft.f64) + (lab.leaf, lab.value, lab.cmp, lab.rel, lab.decisive, stab.stable):
        a.setflags(write=False)
    return Pool(rgb, ft, lab, stab, tau, level)


# ------------------------------------------------------------------------------------------------------------------------
# labels of a whole frame (the zoo's, an oracle-marked frame's on the decode side, a fixture's)
# ------------------------------------------------------------------------------------------------------------------------
FrameLabel = namedtuple("FrameLabel", "ft tex tex_stab m mean clamped lum_leaf lum_value lum_stab")


def label_frame(frame, tau, params=PARAMS):
    """Everything the masks decide about a u8 frame, per block [rows, cols] (stabilities and admitted sets are flat, row-major)."""
    ft = features_of_frame(frame)
    tex = tex_label(ft.a00, ft.dcl, ft.eh, ft.e, params)
    m = ft.ydc.astype(F64) / 8
    mean = float(np.mean(m))
    leaf, value = lum_label(m, mean)
    return FrameLabel(ft, tex, tex_stability(ft.a00, ft.dcl, ft.eh, ft.e, tau, params), m, mean, mean <= orc.L_MIN, leaf, value,
                      lum_stability(m, mean, tau))


def unstable_blocks(fl):
    """[rows, cols] bool: texture or luminance value not decided within tau."""
    return ~(fl.tex_stab.stable & fl.lum_stab.stable).reshape(fl.m.shape)


# ------------------------------------------------------------------------------------------------------------------------
# the zoo: two frames of 16 x 16 blocks
# ------------------------------------------------------------------------------------------------------------------------
ZOO_BLOCKS = 16                # per side: 128 x 128 pixels, 256 blocks
_KY = (0.114, 0.587, 0.299)


def _block_mean(rgb):
    return float(features_of_blocks(rgb[None]).ydc[0]) / 8


def tune_mean(block, target, rng):
    """A block shifted in brightness (all channels, whole levels) and then nudged by +-1 LSB on single samples so that its Y mean
    lands within 0.114 / 64 = 1.8e-3 of ``target``."""
    b = block.astype(np.int16) + int(np.rint(target - _block_mean(block)))
    assert b.min() >= 1 and b.max() <= 254, "tune_mean: the block does not fit at this brightness"
    d = target - _block_mean(b.astype(np.uint8))
    for ch in (1, 2, 0):
        n = int(d * 64 / _KY[ch])                    # truncation: the remainder keeps its sign
        for i in rng.choice(64, abs(n), replace=False):
            b[i // 8, i % 8, ch] += int(np.sign(n))
        d -= n * _KY[ch] / 64
    return b.astype(np.uint8)


def _exact_mean_blocks(level):
    """Two blocks whose pixel mean is exactly ``level``: flat, and rows alternating level -+ 5; the chroma pattern sums to zero."""
    flat = np.full((8, 8, 3), level, np.int16)
    rows = flat.copy()
    rows[0::2] -= 5
    rows[1::2] += 5
    out = []
    for b in (flat, rows):
        b[..., 0] += chroma_pattern()
        assert b.min() >= 0
        out.append(b.astype(np.uint8))
    return out


Zoo = namedtuple("Zoo", "frames labels tau level")


def _pick(mask, order_key, n, prefer_low, window=40):
    """n blocks of ``mask``: of the ``window`` with the smallest ``order_key``, the darkest (prefer_low) or brightest."""
    idx = np.nonzero(mask)[0]
    idx = idx[np.argsort(order_key[idx], kind="stable")][:window]
    m = pool().ft.ydc[idx]
    return list(idx[np.argsort(m if prefer_low else -m, kind="stable")][:n])


def _assemble(clamped, seed):
    p = pool()
    rng = np.random.default_rng(seed)
    lab, stable, m_pool = p.label, p.stab.stable, p.ft.ydc.astype(F64) / 8
    chosen = []
    for k in range(len(COMPARISONS)):
        for side in (False, True):
            ok = stable & lab.decisive[k] & (lab.cmp[k] == side) & (np.abs(lab.rel[k]) <= NEAR) & (m_pool > 30)
            chosen += _pick(ok, np.abs(lab.rel[k]), MIN_SIDE + 1, clamped)
    want_bright = 0
    for i, name in enumerate(TEX_LEAVES):
        if name in TEX_INFEASIBLE:
            continue
        have = int((lab.leaf[chosen] == i).sum())
        # the clamped frame needs blocks above its mean of 90 as well: every other leaf's top-up comes from the bright side there
        bright = (not clamped) or (want_bright % 2 == 0)
        want_bright += 1
        ok = stable & (lab.leaf == i) & ((m_pool > 120) if bright else ((m_pool > 30) & (m_pool < 70)))
        ok[chosen] = False
        chosen += list(rng.choice(np.nonzero(ok)[0], max(0, MIN_LEAF + 2 - have), replace=False))
    unstable = np.nonzero(~stable)[0]
    chosen += list(unstable[np.linspace(0, unstable.size - 1, 12).astype(int)])          # the pool's own tau-unstable blocks
    blocks = [p.rgb[i] for i in chosen]
    # luminance blocks: low-contrast pool blocks moved to the brightness a row needs
    span = p.rgb.reshape(p.rgb.shape[0], -1)
    calm = np.nonzero((lab.leaf == T_INACTIVE) & stable & (m_pool - span.min(1) <= 8.5) & (span.max(1) - m_pool <= 30))[0]
    assert calm.size >= 64, calm.size
    calm = list(rng.permutation(calm)[:64])
    base = lambda: p.rgb[calm.pop()]                  # noqa: E731
    off = 8 * NEAR                                   # 0.008: inside 1e-3 of 15, outside tau / 8
    lum_targets = [15 - off] * MIN_SIDE + [15 + off] * MIN_SIDE + [25 - off] * MIN_SIDE + [25 + off] * MIN_SIDE + \
                  [10.0, 11.0, 12.0, 13.0, 11.5, 12.5] + [19.0, 21.0]
    blocks += [tune_mean(base(), t, rng) for t in lum_targets]
    blocks += _exact_mean_blocks(15) + _exact_mean_blocks(25)
    n_mean = 2 * MIN_SIDE + 1
    mean_bases = [base() for _ in range(n_mean)]
    n_fill = ZOO_BLOCKS ** 2 - len(blocks) - n_mean
    assert n_fill >= 0, f"the zoo does not fit: {len(blocks) + n_mean} blocks"
    ok = stable & ((m_pool < 50) if clamped else (m_pool > 150)) & (m_pool > 30)
    blocks += [p.rgb[i] for i in rng.choice(np.nonzero(ok)[0], n_fill, replace=False)]
    perm = rng.permutation(ZOO_BLOCKS ** 2)

    def frame_of(mean_blocks):
        allb = np.stack(blocks + mean_blocks)[perm].reshape(ZOO_BLOCKS, ZOO_BLOCKS, 8, 8, 3)
        return np.ascontiguousarray(allb.transpose(0, 2, 1, 3, 4).reshape(ZOO_BLOCKS * 8, ZOO_BLOCKS * 8, 3))

    target = 90.0
    moff = 30 * NEAR                                 # 0.03: inside 1e-3 of a mean >= 90, outside 2 tau / 8
    offs = [-moff] * MIN_SIDE + [moff] * MIN_SIDE + [0.0]
    for _ in range(6 if not clamped else 1):         # the unclamped mean depends on these very blocks: iterate to the fixed point
        mean_blocks = [tune_mean(b, target + o, np.random.default_rng(seed + 1 + j)) for j, (b, o) in enumerate(zip(mean_bases, offs))]
        frame = frame_of(mean_blocks)
        if not clamped:
            target = float(np.mean(features_of_frame(frame).ydc.astype(F64) / 8))
    if clamped:                                      # the block that equals the clamped mean: flat 90
        flat = np.full((8, 8, 3), 90, np.int16)
        flat[..., 0] += chroma_pattern()
        mean_blocks[-1] = flat.astype(np.uint8)
        frame = frame_of(mean_blocks)
    frame.setflags(write=False)
    return frame


def zoo_rows(fl):
    """The zoo's coverage table for one labelled frame: {row name: count of tau-stable blocks}, rows = texture leaves, both sides
    of the 13 texture comparisons (decisive, within NEAR), luminance leaves, both sides of 15 / 25 / the frame mean (within NEAR),
    and the deliberately unstable blocks."""
    rows = {}
    ts, ls = fl.tex_stab.stable, fl.lum_stab.stable
    leaf = fl.tex.leaf.reshape(-1)
    for i, name in enumerate(TEX_LEAVES):
        rows["tex:" + name] = int(((leaf == i) & ts).sum())
    for k, (label, _, _) in enumerate(COMPARISONS):
        dec, c, rel = (fl.tex.decisive[k].reshape(-1), fl.tex.cmp[k].reshape(-1), fl.tex.rel[k].reshape(-1))
        for side in (False, True):
            rows[f"cmp:{label}:{'yes' if side else 'no'}"] = int((ts & dec & (c == side) & (np.abs(rel) <= NEAR)).sum())
    m, lleaf = fl.m.reshape(-1), fl.lum_leaf.reshape(-1)
    kind = "clamped" if fl.clamped else "unclamped"
    for i, name in enumerate(LUM_LEAVES):
        rows[f"lum:{kind}:{name}"] = int(((lleaf == i) & ls).sum())
    for name, t in (("15", 15.0), ("25", 25.0), ("mean", max(fl.mean, float(orc.L_MIN)))):
        rel = (m - t) / t
        rows[f"lum:{kind}:m<{name}"] = int((ls & (rel < 0) & (rel >= -NEAR)).sum())
        rows[f"lum:{kind}:m>={name}"] = int((ls & (rel >= 0) & (rel <= NEAR)).sum())
    rows["unstable:tex"] = int((~ts).sum())
    rows["unstable:lum"] = int((~ls).sum())
    for name, t in (("15", 15.0), ("25", 25.0), ("mean", max(fl.mean, float(orc.L_MIN)))):
        rows[f"unstable:m=={name}"] = int((~ls & (np.abs(m - t) <= 2e-3)).sum())
    return rows


def assert_zoo_rows(rows):
    """The coverage conditions; the generator cannot silently lose a row."""
    for name, n in rows.items():
        kind = name.split(":")[0]
        if kind == "tex":
            if name[4:] in TEX_INFEASIBLE:
                assert n == 0, name
            else:
                assert n >= MIN_LEAF, (name, n)
        elif kind == "cmp":
            assert n >= MIN_SIDE, (name, n)
        elif kind == "lum":
            assert n >= (MIN_LEAF if name.split(":")[2] in LUM_LEAVES else MIN_SIDE), (name, n)
        elif name in ("unstable:m==15", "unstable:m==25"):
            assert n >= 2, (name, n)                 # flat and non-flat
        else:
            assert n >= 1, (name, n)


@functools.lru_cache(maxsize=None)
def zoo():
    """-> Zoo(frames = (clamped, unclamped) u8 [128, 128, 3], labels = their FrameLabels, tau, level).  Coverage is asserted here,
    so every user of the zoo holds it."""
    p = pool()
    frames = (_assemble(True, POOL_SEED + 100), _assemble(False, POOL_SEED + 200))
    labels = tuple(label_frame(f, p.tau) for f in frames)
    assert labels[0].clamped and labels[0].mean < orc.L_MIN - 1 and not labels[1].clamped and labels[1].mean > orc.L_MIN + 1
    for fl in labels:
        assert np.abs(fl.ft.c21).min() >= C21_FLOOR
        assert_zoo_rows(zoo_rows(fl))
    return Zoo(frames, labels, p.tau, p.level)


# ------------------------------------------------------------------------------------------------------------------------
# the oracle under a given per-block mask (for blocks whose mask value the statement leaves open)
# ------------------------------------------------------------------------------------------------------------------------
def oracle_encode_yuv(yuv, wm, alpha, mask=None):
    """DctEncoderOracle.encode on a float32 YUV frame (changed in place and returned, as the reference does); ``mask`` ([rows, cols]
    float64 tex * lum, NaN = the oracle's own) replaces the mask per block.  Every step after the masks is per block, so a block
    marked under another mask value is what the reference writes when its tree decides that value.
    -> (yuv, debug dict with mask, c21_pre, c21_post)."""
    ycoef = orc.dct8x8(orc.to_blocks(yuv[:, :, 0]))
    own = orc.texture_mask_vec(None, ycoef) * orc.luminance_mask_vec(None, ycoef)
    use = own if mask is None else np.where(np.isnan(mask), own, mask)
    rows, cols = use.shape
    ucoef = orc.dct8x8(orc.to_blocks(yuv[:, :, 1]))
    pre = ucoef[..., 2, 1].copy()
    post = orc.qim_embed(pre, alpha * use, np.asarray(wm).reshape(-1)[: rows * cols].reshape(rows, cols))
    ucoef[..., 2, 1] = post
    orc.from_blocks(orc.idct8x8(ucoef), yuv[:, :, 1])
    return yuv, dict(mask=use, c21_pre=pre, c21_post=post)


def oracle_mark(frame, wm, alpha, mask=None):
    """mark_frame (embedder.py:33-39) over oracle_encode_yuv.  -> (marked u8 frame, debug dict)."""
    yuv, dbg = oracle_encode_yuv(orc.bgr2yuv_f32(frame.astype(F32)), wm, alpha, mask)
    return np.around(np.clip(orc.yuv2bgr_f32(yuv), a_min=0, a_max=255)).astype(np.uint8), dbg


def oracle_read(frame, alpha, mask=None):
    """check_frame with DctDecoderOracle under a per-block mask override (NaN = the oracle's own).
    -> (bits [rows * cols], x = c21 / step float64 [rows * cols])."""
    yuv = orc.bgr2yuv_f32(frame.astype(F32))
    ycoef = orc.dct8x8(orc.to_blocks(yuv[:, :, 0]))
    own = orc.texture_mask_vec(None, ycoef) * orc.luminance_mask_vec(None, ycoef)
    use = own if mask is None else np.where(np.isnan(mask), own, mask)
    c21 = orc.dct8x8(orc.to_blocks(yuv[:, :, 1]))[..., 2, 1]
    return orc.qim_read(c21, alpha * use).reshape(-1), (c21.astype(F64) / (alpha * use)).reshape(-1)


def device_choice(fl, tex, lum, tau, what=""):
    """Hold a device's tex / lum planes ([rows, cols] float64) against a labelled frame: on every tau-stable block the oracle's
    value within 2e-6 (zero budget), on unstable blocks a member of the admitted set.  -> the mask the device chose per block, as
    the statement spells it: NaN on stable blocks (the oracle's own value), the nearest admitted tex * lum elsewhere."""
    rows, cols = fl.m.shape
    choice = np.full(rows * cols, np.nan)
    picked = {}
    for name, got, ref, stab, slack in (("tex", tex, fl.tex.value, fl.tex_stab, tex_ramp_slack(tau)),
                                        ("lum", lum, fl.lum_value, fl.lum_stab, lum_ramp_slack(tau))):
        got, ref = np.asarray(got, F64).reshape(-1), np.asarray(ref, F64).reshape(-1)
        off = np.abs(got - ref) > 2e-6
        bad = np.nonzero(off & stab.stable)[0]
        assert bad.size == 0, f"{what}: {name} differs on {bad.size} tau-stable blocks, first {bad[:5]}: {got[bad[:5]]} vs {ref[bad[:5]]}"
        vals = ref.copy()
        for i, adm in stab.admitted.items():
            assert in_admitted(got[i], adm, slack), f"{what}: {name} of unstable block {i} is {got[i]!r}, admitted {adm}"
            vals[i] = nearest_admitted(got[i], adm)
        picked[name] = vals
    unstable = ~(fl.tex_stab.stable & fl.lum_stab.stable)
    choice[unstable] = (picked["tex"] * picked["lum"])[unstable]
    return choice.reshape(rows, cols)


# ------------------------------------------------------------------------------------------------------------------------
# the existing DCT fixtures (for the census: which leaves the suite reached before the zoo)
# ------------------------------------------------------------------------------------------------------------------------
def fixture_frames():
    """(name, u8 frame) of every DCT fixture of the parity tests: the stored vectors, the three synthetic 1080p frames and
    test_gpu_sweeps.py's eight extreme frames."""
    import os
    from conftest import GOLDEN, golden_cases
    for case in golden_cases():
        yield case, np.load(os.path.join(GOLDEN, case + ".npz"))["frame"]
    for seed in (2000, 2001, 2003):
        yield f"synthetic_1080p_{seed}", orc.synthetic_frame(1080, 1920, seed)
    from test_gpu_sweeps import _extreme_frames
    for name, frame in _extreme_frames(96, 128, np.random.default_rng(31)).items():
        yield "extreme_" + name, frame


@functools.lru_cache(maxsize=None)
def fixture_features():
    """{name: (a00, dcl, eh, e) flat float32} of fixture_frames()."""
    out = {}
    for name, frame in fixture_frames():
        ft = features_of_frame(frame)
        out[name] = tuple(np.ascontiguousarray(x.reshape(-1)) for x in (ft.a00, ft.dcl, ft.eh, ft.e))
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the stored zoo: the generator's output, kept under tests/golden/ so that the GPU tests do not pay for the pool
# ------------------------------------------------------------------------------------------------------------------------
def _stored_paths():
    import os
    from conftest import GOLDEN
    return os.path.join(GOLDEN, "mask_leaves_zoo.npy"), os.path.join(GOLDEN, "mask_leaves_tau.npy")


@functools.lru_cache(maxsize=None)
def stored_zoo():
    """The zoo as stored (frames u8 [2, 128, 128, 3]; tau and the oracle's level): labelled afresh, coverage asserted afresh.
    test_mask_leaves_statement.py holds the files against zoo(), byte for byte."""
    fpath, tpath = _stored_paths()
    frames = np.load(fpath)
    tau, level = (float(v) for v in np.load(tpath))
    frames.setflags(write=False)
    labels = tuple(label_frame(f, tau) for f in frames)
    assert labels[0].clamped and not labels[1].clamped
    for fl in labels:
        assert np.abs(fl.ft.c21).min() >= C21_FLOOR
        assert_zoo_rows(zoo_rows(fl))
    return Zoo(tuple(frames), labels, tau, level)
