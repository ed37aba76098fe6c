"""Shared by the repeated-singular-value tests of the DwtDctSvd codec (test_svd_repeated_statement.py, test_gpu_svd_repeated.py,
test_kernel_arithmetic.py): what the reference admits for a block whose top singular value is repeated or lies next to a
quantisation threshold, the block families that exercise it, and float32 frames that carry them.

Statement.  The reference replaces the top singular value of the LL block B (blk x blk) by
    s0'(q) = (q + 0.25 + 0.5 bit) scale,   q = s0 // scale
and writes u diag(s') v back from whatever pair LAPACK returned (dwt_dct_svd_encoder.py:41-45).  With B = U diag(sigma) V^T in
float64 the admitted results are therefore
    A(y, q) = B + (s0'(q) - |B y|) (B y / |B y|) y^T
for every unit y in the span of the right singular vectors of the CLUSTER C = {i : sigma_i >= sigma_0 (1 - KAPPA)}: inside the
cluster any orthonormal basis is a valid answer of the decomposition, and A(y, q) is what writing back does to the pair (B y / |B y|, y).
  KAPPA = 2^-20.  Singular values a few float32 ulps apart are one value to float32 LAPACK as much as to the kernels: both
      compute in float32 (ulp 2^-23 relative), and a backward error of a few ulps moves sigma_0 and sigma_1 across each other.
  q = floor(sigma_0 / scale); where sigma_0 lies within ``nu`` of a multiple of scale the neighbouring floor is admitted too
      (nu: ten times the error float32 LAPACK itself shows on the family; the tests compute it from the oracle).
  sigma_0 = 0 (a zero block) admits LAPACK's u0 = v0 = e0: A = s0'(0) e0 e0^T.
nearest_admitted() finds, for a marked block, the nearest member of that set and how far it is."""
from collections import namedtuple

import numpy as np

import offmark_oracle as orc

F = np.float32
KAPPA = 2.0 ** -20
GAMMAS = (2.0 ** -23, 2.0 ** -21, 2.0 ** -17, 2.0 ** -14, 2.0 ** -10, 2.0 ** -7)     # near-gamma family: the first two lie inside KAPPA
EPSILONS = (0.0, 1.0, -1.0, 1e-5, -1e-5, 1e-4, -1e-4, 1e-2, -1e-2)                     # threshold family; +-1.0 stands for +-1 float32 ulp

Nearest = namedtuple("Nearest", "A d resid top q cluster below snew")


def s_new(q, bit, scale):
    return (np.asarray(q, np.float64) + 0.25 + 0.5 * np.asarray(bit, np.float64)) * scale


def cluster_size(B):
    s = np.linalg.svd(np.asarray(B, np.float64), compute_uv=False)
    return (s >= s[..., :1] * (1 - KAPPA)).sum(-1)


def nearest_admitted(B, scale, bit, B_marked, nu=0.0):
    """B, B_marked: [N, n, n] (or one block) float32 LL blocks before / after the marking; bit: [N].  Per block the nearest admitted
    A(y, q) and the metrics: d = max |B_marked - A|, resid = the second singular value of Delta = B_marked - B (an admitted result
    is a rank-one change), top = | sigma_top(B_marked) - sigma_top(A) |, which is | sigma_top(B_marked) - s0'(q) | wherever
    s0'(q) is A's top value (``below`` False; the statement test holds sigma_top(A) == s0' there), q, the cluster size, and below =
    s0'(q) is smaller than another singular value of A (the marked value is not the top one: the reference loses the bit)."""
    B = np.asarray(B, np.float64)
    Bm = np.asarray(B_marked, np.float64)
    single = B.ndim == 2
    if single:
        B, Bm = B[None], Bm[None]
    N, n, _ = B.shape
    bit = np.broadcast_to(np.asarray(bit, np.float64).reshape(-1), (N,))
    U, S, Vt = np.linalg.svd(B)
    inC = S >= S[:, :1] * (1 - KAPPA)                                     # [N, n]
    D = Bm - B
    Ud, Sd, Vdt = np.linalg.svd(D)
    x = Vdt[:, 0, :]                                                      # Delta's top right singular vector
    coef = np.einsum("nij,nj->ni", Vt, x) * inC                           # its coordinates in the cluster's basis
    flat = np.linalg.norm(coef, axis=1) < 1e-6                            # Delta has no direction there: take LAPACK's own v0
    coef[flat] = 0
    coef[flat, 0] = 1
    y = np.einsum("ni,nij->nj", coef, Vt)
    y /= np.linalg.norm(y, axis=1, keepdims=True)
    By = np.einsum("nij,nj->ni", B, y)
    nBy = np.linalg.norm(By, axis=1)
    zero = S[:, 0] == 0
    u = np.where(zero[:, None], np.eye(n)[0][None], By / np.where(zero, 1.0, nBy)[:, None])
    y = np.where(zero[:, None], np.eye(n)[0][None], y)
    nBy = np.where(zero, 0.0, nBy)
    q0 = np.floor(S[:, 0] / scale)
    top_marked = np.linalg.svd(Bm, compute_uv=False)[:, 0]
    best = None
    for dq in (0, -1, 1):
        q = q0 + dq
        if dq == -1:
            ok = (S[:, 0] - q0 * scale <= nu) & (q0 >= 1)
        elif dq == 1:
            ok = (q0 + 1) * scale - S[:, 0] <= nu
        else:
            ok = np.ones(N, bool)
        sn = s_new(q, bit, scale)
        A = B + (sn - nBy)[:, None, None] * u[:, :, None] * y[:, None, :]
        d = np.where(ok, np.abs(Bm - A).reshape(N, -1).max(1), np.inf)
        if best is None:
            best = [A, d, q.copy(), sn.copy()]
        else:
            take = d < best[1]
            best[0][take], best[1][take], best[2][take], best[3][take] = A[take], d[take], q[take], sn[take]
    top_A = np.linalg.svd(best[0], compute_uv=False)[:, 0]
    below = top_A > best[3] * (1 + 1e-12) + 1e-12
    out = Nearest(best[0], best[1], Sd[:, 1], np.abs(top_marked - top_A), best[2], inC.sum(1), below, best[3])
    return Nearest(*(v[0] for v in out)) if single else out


# ---- families ------------------------------------------------------------------------------------------------------------------
def _orth(rng, n):
    q, r = np.linalg.qr(rng.normal(size=(n, n)))
    return q * np.sign(np.diag(r))


def _top(rng, scale, mag, frac=(0.02, 0.08)):
    """A top singular value below ``mag`` whose remainder mod scale lies in frac * scale.  The default puts it just above a multiple:
    either bit moves the value UP, by >= 0.17 scale, so a repeated top value stays below the marked one and the payload survives."""
    k = rng.integers(2, max(3, int(mag / scale) - 1))
    return (k + rng.uniform(*frac)) * scale


def _rotated(rng, s):
    n = len(s)
    return _orth(rng, n) @ np.diag(s) @ _orth(rng, n).T


def _rest(rng, s0, n, hi=0.8):
    """n singular values below s0, each 0.1 .. hi of the previous one (well separated)."""
    out, s = [], s0
    for _ in range(n):
        s = s * rng.uniform(0.1, hi)
        out.append(s)
    return out


Family = namedtuple("Family", "name blocks bits tags")       # blocks [N, n, n] float32, bits [N] u8, tags: one string per block


def families(blk, scale, mag, seed=0, n_rand=48):
    """The seeded block families for one channel: blk in (4, 8), quantisation step ``scale``, top singular values below ``mag``.
    Every family is a Family(name, blocks, bits, tags); bits are chosen so that |s0' - sigma_0| >= 1 (asserted by the statement
    test), i.e. the marking has a direction to compare."""
    n = blk
    rng = np.random.default_rng([seed, blk, int(scale * 16), int(mag)])
    out = []

    def add(name, items):
        blocks = np.array([b for b, _, _ in items]).astype(F)
        bits = np.array([bit for _, bit, _ in items], np.uint8)
        out.append(Family(name, blocks, bits, [t for _, _, t in items]))

    bit_rng = np.random.default_rng([99, blk])         # the bits do not depend on the channel: a tile's bit is shared by its channels

    def rbit():
        return int(bit_rng.integers(0, 2))

    # control: well separated random spectra
    add("control", [(_rotated(rng, [s0] + _rest(rng, s0, n - 1)), rbit(), "rand") for s0 in (_top(rng, scale, mag) for _ in range(n_rand))])

    # axis: a I, diag(a, a, b, c, ...) on permuted axes, a P for permutation matrices P, with signs
    items = []
    for k in range(n_rand // 3):
        a = _top(rng, scale, mag)
        items.append((a * np.eye(n), rbit(), "aI"))
        d = np.array([a, a] + _rest(rng, a, n - 2))
        P, Q = np.eye(n)[rng.permutation(n)], np.eye(n)[rng.permutation(n)]
        items.append((P @ np.diag(d) @ Q, rbit(), "diag_perm"))
        items.append((a * np.eye(n)[rng.permutation(n)] * rng.choice([-1.0, 1.0], (1, n)), rbit(), "aP"))
    add("axis", items)

    # kron: a kron(P, J) and a kron(J, P), P a signed k x k permutation, J the all-ones m x m block: the top value m a has multiplicity
    # k and its eigenspace is off axis.  The first two tiles are the worked case of test_svd_repeated_statement.py: 4x4-pixel squares of 23 placed diagonally.
    items = []
    worked = n == 4 and scale == 15.0
    for k in ([2] if n == 4 else [2, 4]):
        m = n // k
        J = np.ones((m, m))
        first = True
        for trial in range(n_rand // (2 if n == 4 else 4)):
            a = 46.0 if (first and worked) else _top(rng, scale, mag) / m
            P = np.eye(k) if first else np.eye(k)[rng.permutation(k)] * rng.choice([-1.0, 1.0], (1, k))
            for Bk, tag in ((np.kron(P, J), "PxJ"), (np.kron(J, P), "JxP")):
                if first:                                      # bits 0 and 1 on the same block: the payload pair
                    if tag == "PxJ":
                        items.append((a * Bk, 0, tag + ("_worked" if worked else "_k%d" % k)))
                        items.append((a * Bk, 1, tag + ("_worked" if worked else "_k%d" % k)))
                else:
                    items.append((a * Bk, rbit(), "%s_k%d" % (tag, k)))
            first = False
    add("kron", items)

    # rotated-exact: Q1 diag(s, s, ...) Q2^T rounded to float32; double, triple and full multiplicity
    items = []
    for k in range(n_rand):
        mult = (2, 3, n)[k % 3]
        s0 = _top(rng, scale, mag)
        items.append((_rotated(rng, [s0] * mult + _rest(rng, s0, n - mult)), rbit(), "mult%d" % mult))
    add("rotated-exact", items)

    # near-gamma: sigma_1 = sigma_0 (1 - gamma)
    items = []
    for k in range(n_rand):
        g = GAMMAS[k % len(GAMMAS)]
        s0 = _top(rng, scale, mag)
        items.append((_rotated(rng, [s0, s0 * (1 - g)] + _rest(rng, s0, n - 2)), rbit(), "g2^%d" % round(np.log2(g))))
    add("near-gamma", items)

    # below: s0' < sigma_1 -- the marked value is no longer the top one (the reference loses the bit too)
    items = []
    for k in range(n_rand // 2):
        s0 = _top(rng, scale, mag, frac=(0.90, 0.96))
        s1 = s0 - rng.uniform(0.02, 0.10) * scale                         # bit 0 writes s0 - >= 0.65 scale, bit 1 s0 - >= 0.15 scale
        mult2 = k % 2 == 0
        items.append((_rotated(rng, [s0, s0 if mult2 else s1] + _rest(rng, s1, n - 2)), rbit(), "double" if mult2 else "simple"))
    add("below", items)

    # threshold: sigma_0 = k scale + eps; exact (axis-aligned, rank 1 and full rank) and rotated
    items = []
    for eps in EPSILONS:
        for rank1 in (True, False):
            for rot in (False, True):
                kk = int(rng.integers(2, max(3, int(mag / scale) - 1)))
                t = np.float64(F(kk * scale))
                if abs(eps) == 1.0:
                    s0 = float(np.nextafter(F(t), F(np.inf if eps > 0 else -np.inf)))
                else:
                    s0 = float(F(t + eps))
                s = [s0] + ([0.0] * (n - 1) if rank1 else _rest(rng, s0, n - 1))
                if rot:
                    Bk = _rotated(rng, s)
                else:
                    Bk = np.eye(n)[rng.permutation(n)] @ np.diag(s) @ np.eye(n)[rng.permutation(n)]
                items.append((Bk, rbit(), "eps%g_%s_%s" % (eps, "r1" if rank1 else "full", "rot" if rot else "axis")))
    add("threshold", items)
    return out


# ---- frames --------------------------------------------------------------------------------------------------------------------
TILES_PER_ROW = 8
FRINGE = (3, 5)          # rows / columns of pixels outside the tile grid (H, W are no multiples of the tile)


def frame_of(blocks_by_channel, blk, seed=0):
    """A float32 YUV frame [H, W, 3] whose tile c carries blocks_by_channel[ch][c] as the Haar LL block of channel ch (each LL entry
    spread over its 2x2 pixels as entry / 2; float32 Haar taps, so the LL the codec sees is haar_ll() of the frame, within an ulp of
    the block).  Channels not named, tiles beyond a family's length and the fringe hold seeded noise."""
    N = max(len(b) for b in blocks_by_channel.values())
    px = 2 * blk
    rows = -(-N // TILES_PER_ROW)
    H, W = rows * px + FRINGE[0], TILES_PER_ROW * px + FRINGE[1]
    rng = np.random.default_rng([seed, blk, N])
    frame = rng.uniform(-100, 300, (H, W, 3)).astype(F)
    for ch, blocks in blocks_by_channel.items():
        for c, Bk in enumerate(blocks):
            i, j = divmod(c, TILES_PER_ROW)
            frame[i * px:(i + 1) * px, j * px:(j + 1) * px, ch] = np.kron(F(0.5) * Bk.astype(F), np.ones((2, 2), F))
    return frame


def haar_ll(frame, ch, blk):
    """The LL blocks [tiles, blk, blk] (float32) of channel ch in tile order, as the reference and the kernels form them."""
    H, W, _ = frame.shape
    ca = np.array(orc.haar_dwt2(frame[: H // 4 * 4, : W // 4 * 4, ch])[0])
    return orc.to_blocks4(ca, blk).reshape(-1, blk, blk)


def tiles_of(frame, blk):
    H, W, _ = frame.shape
    return (H // 4 * 2) // blk, (W // 4 * 2) // blk


def wm_for(frame, bits):
    """A (1, H W // 64) watermark whose entry c is bits[c] (tile c reads entry c, both block sizes); ones beyond."""
    H, W, _ = frame.shape
    wm = np.ones((1, H * W // 64), np.uint8)
    wm[0, : len(bits)] = bits
    return wm


def decode_decision(B_marked, scale):
    """The float64 read-out of LL blocks, and the distance of the top singular value from the nearest decision threshold."""
    s0 = np.linalg.svd(np.asarray(B_marked, np.float64), compute_uv=False)[..., 0]
    r = np.mod(s0, scale)
    dist = np.minimum(np.minimum(r, scale - r), np.abs(r - 0.5 * scale))
    return (r > 0.5 * scale).astype(np.uint8), dist, s0


# ---- the test frames, the reference levels and the device check --------------------------------------------------------------------
# per block size and YUV channel: (quantisation step, bound of the top singular values): Y reaches 2040 / 4080 for u8 content, U and V ~900 / 1800
SETUP = {4: {0: (7.0, 2040.0), 1: (15.0, 900.0), 2: (21.0, 900.0)}, 8: {0: (7.0, 4080.0), 1: (15.0, 1800.0), 2: (21.0, 1800.0)}}
SCALE_SETS = ((0.0, 15.0, 0.0), (7.0, 15.0, 0.0), (7.0, 15.0, 21.0))          # one, two and three marked channels
FACTOR = 10.0            # the project's convention (test_gpu_svd.py): ~10x what the reference itself shows

Build = namedtuple("Build", "blk frame wm bits fam tags names")      # fam: family index per tile, names: the family names
_cache = {}


def build(blk):
    """One float32 YUV frame per block size carrying every family in all three channels (each channel its own blocks, designed for
    its own step; the watermark bit of a tile is shared, as in the codec), the (1, H W // 64) watermark, and the tile -> family map."""
    if ("build", blk) in _cache:
        return _cache[("build", blk)]
    per_ch = {ch: families(blk, *SETUP[blk][ch], seed=ch) for ch in range(3)}
    names = [f.name for f in per_ch[1]]
    assert all([len(f.blocks) for f in per_ch[ch]] == [len(f.blocks) for f in per_ch[1]] for ch in range(3))
    fam = np.concatenate([np.full(len(f.blocks), i) for i, f in enumerate(per_ch[1])])
    tags = [t for f in per_ch[1] for t in f.tags]
    bits = np.concatenate([f.bits for f in per_ch[1]])                       # channel 1's draw, for all channels
    frame = frame_of({ch: np.concatenate([f.blocks for f in per_ch[ch]]) for ch in range(3)}, blk, seed=7)
    out = Build(blk, frame, wm_for(frame, bits), bits, fam, tags, names)
    _cache[("build", blk)] = out
    return out


def measure(b, scales, marked, nu_by_ch):
    """-> {ch: Nearest} of a marked frame against the statement, per marked channel, over the family tiles."""
    n = len(b.bits)
    return {ch: nearest_admitted(haar_ll(b.frame, ch, b.blk)[:n], scales[ch], b.bits, haar_ll(marked, ch, b.blk)[:n], nu_by_ch[ch])
            for ch in range(3) if scales[ch] > 0}


EPS32 = 2.0 ** -24       # float32 unit roundoff


def format_term(b, ch, scale):
    """What float32 itself cannot resolve, per tile; non-zero only on the near-gamma tiles OUTSIDE the cluster (gamma = 2^-17 ... 2^-7).
    A float32 solver is at best backward stable: it decomposes B + E with |E| ~ EPS32 sigma_0, and a perturbation of that size turns
    the top singular pair towards a neighbour at relative distance gamma by the angle EPS32 / gamma (Wedin); the marking
    (s0' - sigma_0) u0 v0^T then moves by that angle times |s0' - sigma_0|.  At gamma = 2^-17 that is 2^-7 |s0' - sigma_0| ~ 0.04, far above
    the few-ulp level of every other family.  The reference level says little there: numpy's linalg.svd decomposes a float32 block
    in float64 LAPACK and rounds the factors, so the only float32 perturbation the oracle's vectors see is the rounding of its DCT
    and Haar steps -- one random draw per tile of the same EPS32 / gamma law, and 10 x the largest of 8 draws does not bound the
    largest of another 8 (measured on the device: blk 8, channel 0, gamma = 2^-17: d = 2.4e-2 against a reference level of 1.6e-3; blk 4
    channel 1: 5.4e-3 against 4.4e-3).  So these tiles, and only these, are allowed FACTOR x this term on top of FACTOR x the level."""
    n = len(b.bits)
    s = np.linalg.svd(haar_ll(b.frame, ch, b.blk)[:n].astype(np.float64), compute_uv=False)
    gap = 1 - s[:, 1] / np.maximum(s[:, 0], 1e-300)
    move = np.abs(s_new(np.floor(s[:, 0] / scale), b.bits, scale) - s[:, 0])
    near = (b.fam == b.names.index("near-gamma")) & (gap > KAPPA)
    return np.where(near, EPS32 / np.maximum(gap, EPS32) * move, 0.0)


def reference(blk, scales):
    """The oracle's own marked frame of build(blk) with ``scales``, its metrics, nu per channel and family, and the reference levels
    {(family, ch, metric): max over the family's tiles}.  Computed once per (blk, scales)."""
    key = ("ref", blk, tuple(scales))
    if key in _cache:
        return _cache[key]
    b = build(blk)
    enc = orc.DwtDctSvdEncoderOracle(scales=scales, blk=blk)
    enc.read_wm(b.wm)
    marked = enc.encode(b.frame.copy())
    n = len(b.bits)
    nu = {}
    for ch in range(3):
        if scales[ch] > 0:
            s64 = np.linalg.svd(haar_ll(b.frame, ch, blk)[:n].astype(np.float64), compute_uv=False)[:, 0]
            err = np.abs(enc.debug_ch[ch]["s0"].reshape(-1)[:n].astype(np.float64) - s64)
            nu[ch] = FACTOR * np.array([err[b.fam == i].max() for i in range(len(b.names))])[b.fam]      # per tile: its family's
    m = measure(b, scales, marked, nu)
    levels = {(name, ch, metric): float(getattr(m[ch], metric)[b.fam == i].max())
              for i, name in enumerate(b.names) for ch in m for metric in ("d", "resid", "top")}
    out = dict(marked=marked, metrics=m, nu=nu, levels=levels)
    _cache[key] = out
    return out


def check(b, scales, ref, marked, label, out=print):
    """A marked frame against the statement, with the tolerances of test_gpu_svd_repeated.py: per family, channel and metric at most FACTOR x
    max(the family's reference level, the control family's); d of the near-gamma tiles outside the cluster additionally FACTOR x
    format_term() (see there for why, with the measured numbers); | sigma_top - s0' | at most scale / 64 whatever the factor.  Prints one row per family and channel and
    returns the list of violations (strings)."""
    m = measure(b, scales, marked, ref["nu"])
    bad = []
    for ch, r in m.items():
        extra = FACTOR * format_term(b, ch, scales[ch])
        for i, name in enumerate(b.names):
            sel = b.fam == i
            row = f"{label} blk{b.blk} scales={tuple(scales)} ch{ch} {name:14s} tiles={int(sel.sum()):3d}"
            for metric in ("d", "resid", "top"):
                lvl = ref["levels"][(name, ch, metric)]
                bound = FACTOR * max(lvl, ref["levels"][("control", ch, metric)])
                val = getattr(r, metric)[sel]
                tol = min(bound, scales[ch] / 64) if metric == "top" else bound + (extra[sel] if metric == "d" else 0.0)
                row += f" | {metric}: ref {lvl:.2e} got {val.max():.2e} bound {bound:.2e}"
                worst = int(np.argmax(val - tol))
                if (val > tol).any():
                    bad.append(f"{row.split('|')[0]}{metric} {val[worst]:.3e} > {np.broadcast_to(tol, val.shape)[worst]:.3e} "
                               f"(tile tag {np.array(b.tags)[sel][worst]}, {int((val > tol).sum())} tiles)")
            if name == "near-gamma":
                row += f" | float32 term on gamma >= 2^-17 tiles <= {extra[sel].max():.2e}"
            out(row)
    return bad


# ---- u8 RGB tiles whose oracle LL (channel 1) has a repeated top singular value ---------------------------------------------------
# The LL entry of a 2x2 group of one colour is a fixed float32 function of the colour (bgr2yuv_f32, then the Haar taps; the kernels
# form it from the 2x2 channel sums, ll_of_sums -- another fixed function of the colour).  So a tile painted with two colours, B on
# the diagonal groups and A elsewhere, has the LL block a J + (b - a) I EXACTLY, whatever floats a and b are, in the oracle's
# arithmetic and in the kernels' alike: singular values |b - a| (blk - 1 times) and |(blk - 1) a + b|.  Colours with
# |b - a| > |(blk - 1) a + b| give a top singular value of multiplicity blk - 1 ("multi": 3 for blk 4, 7 for blk 8), exactly.
# An exact FULL multiplicity would need b = -a, which the conversion's lattice does not contain (U = 0.492 (c0 - Y) + 0.5 makes
# a + b a multiple of 0.000984 plus 2): the closest pairs ("nearfull") have |a + b| ~ 3e-4, all blk values within ~1e-5 relative.
U8Tiles = namedtuple("U8Tiles", "blk frame wm bits tags sigma")


def _ll_of_colour(c):
    """Oracle LL entry (channel 1) of a 2x2 group of colour c [..., 3] (u8 values)."""
    u = orc.bgr2yuv_f32(np.asarray(c, F))[..., 1]
    lo = u * orc._HAAR + u * orc._HAAR
    return lo * orc._HAAR + lo * orc._HAAR


U8_SCALE = {4: 24.0, 8: 30.0}      # the u8 rounding of a 16x16 tile moves its singular values more: a step whose quarter stays above twice that


def u8_tiles(blk, count=24, down=False):
    """-> U8Tiles: a u8 RGB frame (no fringe, H and W multiples of 16) of ``count`` "multi" tiles and, blk 4, ``count`` "nearfull"
    ones, the watermark, and each tile's float64 singular values (of the oracle's LL).  Asserted here: the LL block is a J + (b - a) I
    (rows permuted on every other tile), the cluster has the size claimed, and the top value sits 0.03 .. 0.2 of a step above a
    multiple of U8_SCALE[blk] (clear of the floor threshold; either bit moves it up, so the repeated value stays below the marked
    one and the payload survives); colours keep 40 levels from 0 and 255 so that no marked pixel clips.
    ``down`` (blk 4): 4 x ``count`` "nearfull" tiles whose remainder lies anywhere in 0.3 .. 0.999 of a step, with the bit that sends
    the mark BELOW the other three values (0 below 0.8, either above): the marked spectrum has three top values within ~0.3 %
    (the u8 rounding splits them) that were never moved, so they sit anywhere, also next to a read-out threshold."""
    if ("u8", blk, down) in _cache:
        return _cache[("u8", blk, down)]
    assert blk == 4 or not down
    scale = U8_SCALE[blk]
    rng = np.random.default_rng([5, blk])
    n = blk
    g = np.arange(40, 216)
    tiles, tags, sig = [], [], []

    def add(kind, A, Bc):
        a, b = float(_ll_of_colour(A)), float(_ll_of_colour(Bc))
        top = abs(b - a)
        frac = np.mod(top, scale) / scale
        if not ((0.3 < frac < 0.999 if down else 0.03 < frac < 0.2) and top > 3 * scale):
            return False
        cols = np.where(np.eye(n, dtype=bool)[:, :, None], Bc[None, None, :], A[None, None, :]).astype(np.uint8)
        cols = cols[rng.permutation(n)] if len(tiles) % 2 else cols       # a row permutation keeps the singular values
        tile = np.kron(cols.transpose(2, 0, 1), np.ones((2, 2), np.uint8)).transpose(1, 2, 0)      # each LL entry's colour on its 2x2 pixels
        ll = np.array(orc.haar_dwt2(orc.bgr2yuv_f32(tile.astype(F))[:, :, 1])[0])
        assert set(np.unique(ll)) == {F(a), F(b)}
        sv = np.linalg.svd(ll.astype(np.float64), compute_uv=False)
        if kind == "multi":
            assert (sv >= sv[0] * (1 - KAPPA)).sum() == n - 1 and abs(sv[0] - top) <= 1e-9 * top and sv[n - 2] >= sv[0] * (1 - 1e-12)
        else:
            assert sv[n - 1] >= sv[0] * (1 - 2.5e-5)
        tiles.append(tile), tags.append(kind), sig.append(sv)
        return True

    k = count if down else 0
    while k < count:                                                      # multi: |b - a| well above |(n - 1) a + b|
        A, Bc = rng.integers(40, 216, 3), rng.integers(40, 216, 3)
        a, b = float(_ll_of_colour(A)), float(_ll_of_colour(Bc))
        if abs(b - a) > 1.25 * abs((n - 1) * a + b):
            k += add("multi", A, Bc)
    k = 0
    while n == 4 and k < (4 * count if down else count):                  # nearfull: for a random A the colour B of the lattice closest to b = -a
        A = rng.integers(40, 216, 3)
        a = float(_ll_of_colour(A))
        c2 = int(rng.integers(40, 216))
        cand = np.stack(np.meshgrid(g, g, [c2], indexing="ij"), -1).reshape(-1, 3)
        bb = _ll_of_colour(cand).astype(np.float64)
        miss = np.abs(np.abs(bb - a) - np.abs(3 * a + bb)) / np.maximum(np.abs(bb - a), 1e-9)
        j = int(np.argmin(miss))
        if miss[j] < 2e-5:
            k += add("nearfull", A, cand[j])
    per_row = 8
    while len(tiles) % per_row:
        tiles.append(tiles[0]), tags.append(tags[0]), sig.append(sig[0])
    px = 2 * blk
    rows = len(tiles) // per_row
    frame = np.concatenate([np.concatenate(tiles[r * per_row:(r + 1) * per_row], 1) for r in range(rows)], 0)
    bits = rng.integers(0, 2, len(tiles)).astype(np.uint8)
    if down:
        frac = np.mod(np.array(sig)[:, 0], scale) / scale
        bits[frac < 0.8] = 0
        assert (s_new(np.floor(np.array(sig)[:, 0] / scale), bits, scale) < np.array(sig)[:, 3] - 0.04 * scale).all()
    out = U8Tiles(blk, frame, wm_for(frame, bits), bits, tags, np.array(sig))
    assert frame.shape == (rows * px, per_row * px, 3)
    _cache[("u8", blk, down)] = out
    return out


def u8_y_tiles(blk, count=24):
    """-> U8Tiles for channel 0: grey 2x2 groups of value v on black, placed as a permutation matrix (the identity on every other tile).
    Y of black is 0 and Y of a grey is one float y(v), so the LL block is 2 y(v) P exactly: ``blk`` equal singular values.  The top
    value sits 0.03 .. 0.2 of a step above a multiple of U8_SCALE[blk], as in u8_tiles."""
    if ("u8y", blk) in _cache:
        return _cache[("u8y", blk)]
    scale = U8_SCALE[blk]
    rng = np.random.default_rng([6, blk])
    n = blk
    tiles, tags, sig = [], [], []
    while len(tiles) < count:
        v = int(rng.integers(40, 236))                                    # the mark adds up to 0.75 step / 2 to a grey pixel: no clipping
        P = np.eye(n, dtype=bool) if len(tiles) % 2 == 0 else np.eye(n, dtype=bool)[rng.permutation(n)]
        tile = np.kron(np.where(P, v, 0).astype(np.uint8), np.ones((2, 2), np.uint8))[:, :, None].repeat(3, 2)
        ll = np.array(orc.haar_dwt2(orc.bgr2yuv_f32(tile.astype(F))[:, :, 0])[0])
        a = float(ll.max())
        if not (0.03 < np.mod(a, scale) / scale < 0.2 and a > 3 * scale):
            continue
        assert np.array_equal(ll, np.where(P, F(a), F(0))) and abs(a - 2 * v) < 1e-3
        sv = np.linalg.svd(ll.astype(np.float64), compute_uv=False)
        assert sv[n - 1] >= sv[0] * (1 - 1e-12) and abs(sv[0] - a) <= 1e-9 * a
        tiles.append(tile), tags.append("aI" if len(tiles) % 2 == 0 else "aP"), sig.append(sv)
    per_row, px = 8, 2 * blk
    rows = len(tiles) // per_row
    frame = np.concatenate([np.concatenate(tiles[r * per_row:(r + 1) * per_row], 1) for r in range(rows)], 0)
    bits = rng.integers(0, 2, len(tiles)).astype(np.uint8)
    out = U8Tiles(blk, frame, wm_for(frame, bits), bits, tags, np.array(sig))
    _cache[("u8y", blk)] = out
    return out


def u8_ll(frame_u8, blk, ch=1):
    """Channel ch's LL blocks of a u8 frame as the reference forms them (float32), in tile order."""
    return haar_ll(orc.bgr2yuv_f32(frame_u8.astype(F)), ch, blk)


def spectrum_error(t, marked_u8, ch=1):
    """Per tile: max | sorted singular values of LL(marked) - sorted {s0', sigma_1, ...} | in float64 (channel ch, step U8_SCALE), s0'
    from the tile's own sigma_0 and bit (its floor is clear of the thresholds by construction)."""
    scale = U8_SCALE[t.blk]
    got = np.linalg.svd(u8_ll(marked_u8, t.blk, ch)[: len(t.bits)].astype(np.float64), compute_uv=False)
    want = t.sigma.copy()
    want[:, 0] = s_new(np.floor(t.sigma[:, 0] / scale), t.bits, scale)
    return np.abs(np.sort(got, 1) - np.sort(want, 1)).max(1)
