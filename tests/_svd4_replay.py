"""svd4_top() and svd_update() of csrc/svd_kernels.hiph line by line in float32 (fma = exact product, one rounding; the kernel's
v_rcp / v_rsq approximations are exact divisions here), written like test_kernel_arithmetic._svd_top_eigenvalue.  The build has
-ffp-contract=off, so only the kernel's explicit fmaf calls fuse.  ``slow_path`` = False replays the solver as it was before
the Jacobi slow path (a vanishing adjugate fell back to e0): the statement tests show the defect on it."""
import os
import re

import numpy as np

from conftest import PKG
from test_kernel_arithmetic import F, _svd_gram, _svd_top_eigenvalue, fma

SRC = open(os.path.join(PKG, "csrc", "svd_kernels.hiph")).read()


def constants():
    tol = float(re.search(r"kTolTight = ([0-9.eE+-]+)f", SRC).group(1))
    cap = int(re.search(r"kCapTight = (\d+)", SRC).group(1))
    noise = re.search(r"kAdjNoise = ([0-9.eE+x/p-]+)f;", SRC)
    jcap = re.search(r"kJacobiCap = (\d+);", SRC)
    jtol = re.search(r"kJacobiTol = ([0-9.eE+x/p-]+)f;", SRC)
    return dict(tol=F(tol), cap=cap, noise=F(float.fromhex(noise.group(1))) if noise else None,
                jcap=int(jcap.group(1)) if jcap else None, jtol=F(float.fromhex(jtol.group(1))) if jtol else None)


def _det3(a, b, c, d, e, f, g, h, i):
    return fma(a, fma(e, i, -(f * h)), fma(-b, fma(d, i, -(f * g)), c * fma(d, h, -(e * g))))


def _cofactor(M, I, J):
    r = [k for k in range(4) if k != I]
    c = [k for k in range(4) if k != J]
    d = _det3(*(M[:, r[i], c[j]] for i in range(3) for j in range(3)))
    return -d if (I + J) & 1 else d


PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def _jacobi_top(M, scale, jtol, jcap):
    """jacobi4_top(): cyclic Jacobi on the symmetric 4x4 M (= G - lam I, full storage) with the rotations accumulated; returns
    the column of the largest diagonal entry (unit length up to rounding) and the sweeps each block took."""
    N = M.shape[0]
    a = M.copy()
    V = np.zeros((N, 4, 4), F)
    for i in range(4):
        V[:, i, i] = 1
    lim = (jtol * scale) * (jtol * scale)
    skip = F(0.25) * (jtol * scale)
    active = np.ones(N, bool)
    sweeps = np.zeros(N, int)
    for _ in range(jcap):
        for p, q in PAIRS:
            apq = a[:, p, q].copy()
            with np.errstate(all="ignore"):
                theta = ((a[:, q, q] - a[:, p, p]) * F(0.5) * (F(1) / apq)).astype(F)
            rot = active & (np.abs(apq) > skip) & ~np.isnan(theta)
            with np.errstate(all="ignore"):
                t = (np.copysign(F(1), theta) / (np.abs(theta) + np.sqrt(fma(theta, theta, F(1))))).astype(F)
                c = (F(1) / np.sqrt(fma(t, t, F(1)))).astype(F)
            t = np.where(rot, t, F(0)).astype(F)
            c = np.where(rot, c, F(1)).astype(F)
            s = (t * c).astype(F)
            app = fma(-t, apq, a[:, p, p])
            aqq = fma(t, apq, a[:, q, q])
            a[:, p, p], a[:, q, q] = app, aqq
            a[:, p, q] = a[:, q, p] = np.where(rot, F(0), apq)
            for r in range(4):
                if r != p and r != q:
                    arp, arq = a[:, r, p].copy(), a[:, r, q].copy()
                    n_p = fma(c, arp, -(s * arq))
                    n_q = fma(s, arp, c * arq)
                    a[:, r, p] = a[:, p, r] = n_p
                    a[:, r, q] = a[:, q, r] = n_q
            for r in range(4):
                vrp, vrq = V[:, r, p].copy(), V[:, r, q].copy()
                V[:, r, p] = fma(c, vrp, -(s * vrq))
                V[:, r, q] = fma(s, vrp, c * vrq)
        sweeps += active
        off = fma(a[:, 2, 3], a[:, 2, 3], fma(a[:, 1, 3], a[:, 1, 3], fma(a[:, 1, 2], a[:, 1, 2],
                  fma(a[:, 0, 3], a[:, 0, 3], fma(a[:, 0, 2], a[:, 0, 2], a[:, 0, 1] * a[:, 0, 1])))))
        active &= off > lim
        if not active.any():
            break
    k = np.zeros(N, int)
    best = a[:, 0, 0].copy()
    for i in range(1, 4):
        take = a[:, i, i] > best
        best = np.where(take, a[:, i, i], best)
        k = np.where(take, i, k)
    return V[np.arange(N), :, k], sweeps


def svd4_top(B, slow_path=True):
    """-> dict(s0, w, v, lam, slow, sweeps): svd4_top()'s Svd4 per block of B [N, 4, 4] float32, the Laguerre eigenvalue, and
    which blocks took the slow path.  A kernel source without the trigger constant has no slow path to replay."""
    B = np.asarray(B, F)
    N = B.shape[0]
    k = constants()
    slow_path = slow_path and k["noise"] is not None
    G = _svd_gram(B)
    lam, _ = _svd_top_eigenvalue(G, k["tol"], k["cap"])
    M = G.copy()
    for i in range(4):
        for j in range(i):
            M[:, i, j] = M[:, j, i]
    for i in range(4):
        M[:, i, i] = M[:, i, i] - lam
    cof = {(i, j): _cofactor(M, i, j) for i in range(4) for j in range(i, 4)}
    col = lambda kk: np.stack([cof[(min(i, kk), max(i, kk))] for i in range(4)], 1)      # noqa: E731
    ks = np.zeros(N, int)
    best = np.abs(cof[(0, 0)])
    for i in range(1, 4):
        take = np.abs(cof[(i, i)]) > best
        best = np.where(take, np.abs(cof[(i, i)]), best)
        ks = np.where(take, i, ks)
    v = np.stack([col(i) for i in range(4)], 1)[np.arange(N), ks]
    with np.errstate(all="ignore"):
        unit = np.where(best > 0, F(1) / best, F(0)).astype(F)
        v = (v * unit[:, None]).astype(F)
        n2 = fma(v[:, 3], v[:, 3], fma(v[:, 2], v[:, 2], fma(v[:, 1], v[:, 1], v[:, 0] * v[:, 0])))
        inv = np.where(n2 > 0, F(1) / np.sqrt(n2), F(0)).astype(F)
    ok = n2 > 0
    e0 = np.zeros((N, 4), F)
    e0[:, 0] = 1
    vv = np.where(ok[:, None], (v * inv[:, None]).astype(F), e0)
    slow = np.zeros(N, bool)
    sweeps = np.zeros(N, int)
    if slow_path:
        with np.errstate(all="ignore"):
            slow = ((best / lam).astype(F) / lam).astype(F) < k["noise"] * lam
        if slow.any():
            vj, sw = _jacobi_top(M[slow], lam[slow], k["jtol"], k["jcap"])
            sweeps[slow] = sw
            m2 = fma(vj[:, 3], vj[:, 3], fma(vj[:, 2], vj[:, 2], fma(vj[:, 1], vj[:, 1], vj[:, 0] * vj[:, 0])))
            with np.errstate(all="ignore"):
                vj = (vj * (F(1) / np.sqrt(m2)).astype(F)[:, None]).astype(F)
            vv[slow] = vj
            ok = ok | slow
    w = np.stack([fma(B[:, i, 3], vv[:, 3], fma(B[:, i, 2], vv[:, 2], fma(B[:, i, 1], vv[:, 1], B[:, i, 0] * vv[:, 0]))) for i in range(4)], 1)
    s0 = np.where(ok, np.sqrt(fma(w[:, 3], w[:, 3], fma(w[:, 2], w[:, 2], fma(w[:, 1], w[:, 1], w[:, 0] * w[:, 0])))), np.sqrt(lam)).astype(F)
    return dict(s0=s0, w=w, v=vv, lam=lam, slow=slow, sweeps=sweeps, best=best)


def marked_ll(B, s0, w, v, bits, scale):
    """svd_update()'s change applied to the LL block: B + 2 dU in float32 (dU is the amount added to each of a 2x2 group's
    pixels, half the LL change), for any solver's (s0, w, v) -- n = 4 or 8."""
    B = np.asarray(B, F)
    n = B.shape[1]
    scale = F(scale)
    with np.errstate(all="ignore"):
        s_new = ((np.floor_divide(s0, scale) + F(0.25) + F(0.5) * bits.astype(F)) * scale).astype(F)
        g = (F(0.5) * (s_new - s0) / s0).astype(F)
    dU = ((g[:, None] * w)[:, :, None] * v[:, None, :]).astype(F)
    zero = ~(s0 > 0)
    z = np.zeros((n, n), F)
    z[0, 0] = 1
    dU[zero] = (F(0.5) * s_new[zero])[:, None, None] * z[None]
    return (B + F(2) * dU).astype(F)
