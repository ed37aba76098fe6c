"""CPU side of the repeated-singular-value tests of the DwtDctSvd codec (no GPU needed): the families of tests/_svd_repeated.py
have the spectra they claim, the oracle's own float32 results satisfy the statement (their per-family maxima are the reference
levels the device is held to, printed with -rP), the oracle's pair override agrees with the plain oracle, and a line-by-line
float32 replay of svd4_top (tests/_svd4_replay.py) stays inside the admitted set on every family.

The defect the replay guards.  svd4_top took its vector from a column of adj(G - lam I), which is the zero matrix for a repeated
top eigenvalue, and fell back to e0.  For the LL block 46 [[J, 0], [0, J]] (two 4x4-pixel squares of 23, placed diagonally; singular
values 92, 92, 0, 0) that gave s0 = |B e0| = 65.05 in place of 92, a marking along a direction that is no singular pair, and a
read-out of [0, 0] where the reference reads [0, 1].  With the solver's slow path the replay reads [0, 1]."""
import numpy as np
import pytest

import _svd4_replay as rp
import _svd_repeated as sr
import offmark_oracle as orc

F = np.float32


@pytest.mark.parametrize("blk", [4, 8])
def test_families_have_the_spectra_they_claim(blk):
    for ch, (scale, mag) in sr.SETUP[blk].items():
        for fam in sr.families(blk, scale, mag, seed=ch):
            S = np.linalg.svd(fam.blocks.astype(np.float64), compute_uv=False)
            size = (S >= S[:, :1] * (1 - sr.KAPPA)).sum(1)
            gap = 1 - S[:, 1] / S[:, 0]
            assert S[:, 0].max() < mag and len(fam.blocks) == len(fam.bits) == len(fam.tags) >= 24
            for i, tag in enumerate(fam.tags):
                what = (fam.name, tag, i, S[i])
                if fam.name == "control":
                    assert size[i] == 1 and gap[i] >= 0.19, what
                elif tag in ("aI", "aP") or tag == "mult%d" % blk:
                    assert size[i] == blk, what
                elif tag in ("diag_perm", "mult2", "double"):
                    assert size[i] == 2 and S[i, 2] <= 0.81 * S[i, 0], what
                elif tag == "mult3":
                    assert size[i] == 3, what
                elif tag == "PxJ_worked":
                    assert np.allclose(S[i], [92, 92, 0, 0], rtol=0, atol=1e-12), what
                elif tag.startswith(("PxJ_k", "JxP_k")):
                    k = int(tag[-1])
                    assert size[i] == k and np.allclose(S[i, k:], 0, atol=1e-9 * S[i, 0]), what
                elif tag.startswith("g2^"):
                    g = 2.0 ** int(tag[3:])
                    assert size[i] == (2 if g < sr.KAPPA else 1) and abs(gap[i] - g) <= 2.0 ** -22, what      # the float32 rounding of the block
                elif tag == "simple":
                    assert size[i] == 1, what
                elif tag.startswith("eps"):
                    eps = float(tag[3:].split("_")[0])
                    k = np.round(S[i, 0] / scale)
                    want = np.nextafter(F(k * scale), F(np.inf if eps > 0 else -np.inf)) - k * scale if abs(eps) == 1 else eps
                    tol = (0 if abs(eps) == 1 else 2.0 ** -23 * S[i, 0]) + (0 if "axis" in tag else 8 * 2.0 ** -24 * S[i, 0])      # the float32 rounding of eps, of the rotated block
                    assert abs((S[i, 0] - k * scale) - want) <= tol, what
                    assert (S[i, 1] == 0 if "r1_axis" in tag else True) and (S[i, 1] > 0.05 * S[i, 0] if "full" in tag else S[i, 1] < 1e-4), what
                else:
                    raise AssertionError(what)
            # the marking has a direction: |s0' - sigma_0| >= 1 for the bit drawn -- next to a threshold for either floor
            q = np.floor(S[:, 0] / scale)
            move = np.abs(sr.s_new(q, fam.bits, scale) - S[:, 0])
            if fam.name == "threshold":
                move = np.minimum(move, np.abs(sr.s_new(np.round(S[:, 0] / scale) - 1, fam.bits, scale) - S[:, 0]))
            assert move.min() >= 1, (fam.name, ch, move.min())
            if fam.name == "below":
                assert (sr.s_new(q, fam.bits, scale) < S[:, 1]).all()
            elif fam.name not in ("threshold",):
                assert (sr.s_new(q, fam.bits, scale) > S[:, 0]).all()          # the marked value stays the top one: the payload survives


@pytest.mark.parametrize("blk", [4, 8])
def test_oracle_results_pass_the_metric_and_set_the_reference_levels(blk):
    """The reference's arithmetic (oracle, float32 factors) on every family: within a few float32 ulps of the nearest admitted result.
    The maxima printed here are the reference levels; the device tests allow 10 x these."""
    b = sr.build(blk)
    for scales in sr.SCALE_SETS:
        ref = sr.reference(blk, scales)
        assert not sr.check(b, scales, ref, ref["marked"], "oracle")          # prints the levels; trivially inside 10 x itself
        for ch, r in ref["metrics"].items():
            mag = sr.SETUP[blk][ch][1]
            ulps = 64 * 2.0 ** -24 * mag                                      # u, s, v, two DCTs and two Haar steps, each rounded to float32
            near = b.fam == b.names.index("near-gamma")
            assert r.d[~near].max() <= ulps and r.resid.max() <= ulps and r.top.max() <= ulps, (scales, ch, r.d[~near].max(), r.resid.max(), r.top.max())
            # outside a cluster but within 2^-14 of it, float32 turns the pair by ~2^-24 / gamma (the reference's DCT rounds the block)
            assert r.d[near].max() <= 64 * 2.0 ** -24 / 2.0 ** -17 * scales[ch], (scales, ch, r.d[near].max())
            assert ((r.snew >= np.linalg.svd(r.A, compute_uv=False)[:, 0] * (1 - 1e-12)) | r.below).all()      # top(A) is s0' unless "below"
            assert r.below[b.fam == b.names.index("below")].all()
            assert not r.below[np.isin(b.fam, [b.names.index(n) for n in ("control", "axis", "kron", "rotated-exact", "near-gamma")])].any()
        # unmarked channels: untouched; the fringe: the reference sends the part of it inside the multiple-of-4 area through its Haar
        # round trip (last float32 bits move), the kernels leave all of it alone
        th, tw = sr.tiles_of(b.frame, blk)
        H, W, _ = b.frame.shape
        for ch in range(3):
            if not scales[ch] > 0:
                assert np.array_equal(ref["marked"][:, :, ch], b.frame[:, :, ch])
        assert np.array_equal(ref["marked"][H // 4 * 4:], b.frame[H // 4 * 4:]) and np.array_equal(ref["marked"][:, W // 4 * 4:], b.frame[:, W // 4 * 4:])
        assert np.abs(ref["marked"][th * 2 * blk:] - b.frame[th * 2 * blk:]).max() <= 1e-4 and np.abs(ref["marked"][:, tw * 2 * blk:] - b.frame[:, tw * 2 * blk:]).max() <= 1e-4


def test_numpy_decomposes_float32_blocks_in_float64():
    """What "the reference level" means: np.linalg.svd of a float32 block is the float64 decomposition rounded to float32, so
    the oracle's vectors carry no float32 solver error -- only the rounding of its factors and of its DCT and Haar steps.  That is
    why the reference level of the near-gamma tiles outside the cluster is no bound for a float32 solver (format_term)."""
    B = sr.families(4, 15.0, 900.0)[0].blocks
    s32 = np.linalg.svd(B, compute_uv=False)
    assert s32.dtype == F and np.array_equal(s32, np.linalg.svd(B.astype(np.float64), compute_uv=False).astype(F))


def test_nearest_admitted_on_constructed_results():
    """The helper itself: an exact admitted result has d = resid = top = 0 (to float64), for any y in the cluster; a result along a
    vector outside the cluster has d of the size of the marking; a zero block admits s0' e0 e0^T; the neighbouring floor is
    admitted only within nu of a threshold."""
    J = np.ones((2, 2))
    B = 46 * np.kron(np.eye(2), J)
    for y in ([1, 1, 0, 0], [0, 0, 1, 1], [1, 1, 1, 1], [1, 1, -2, -2]):
        y = np.array(y, float) / np.linalg.norm(y)
        By = B @ y
        A = B + (101.25 - 92) * np.outer(By / 92, y)
        r = sr.nearest_admitted(B, 15.0, 1, A)
        assert r.d < 1e-10 and r.resid < 1e-10 and r.top < 1e-10 and r.cluster == 2 and r.q == 6 and not r.below
    e0 = np.eye(4)[0]
    A = B + (101.25 - np.linalg.norm(B @ e0)) * np.outer(B @ e0 / np.linalg.norm(B @ e0), e0)        # what the old fallback wrote
    assert sr.nearest_admitted(B, 15.0, 1, A).d > 4
    Z = np.zeros((4, 4))
    A = Z.copy()
    A[0, 0] = 11.25
    assert sr.nearest_admitted(Z, 15.0, 1, A).d == 0
    D = np.diag([30.0 + 1e-5, 3, 2, 1])
    lower = D + np.diag([(1.25 * 15) - D[0, 0], 0, 0, 0])                  # q = 1 instead of 2
    assert sr.nearest_admitted(D, 15.0, 0, lower, nu=1e-4).d < 1e-10 and sr.nearest_admitted(D, 15.0, 0, lower, nu=1e-6).d > 14


def test_oracle_pair_override_agrees_with_the_plain_oracle():
    """DwtDctSvdEncoderOracle(pair_override=...): handed LAPACK's own pair (or nothing) the bytes are the plain oracle's; handed
    another pair of a repeated top value's eigenspaces the result is another member of the admitted set."""
    blk = 4
    b = sr.build(blk)
    scales = (0.0, 15.0, 0.0)
    ref = sr.reference(blk, scales)
    th, tw = sr.tiles_of(b.frame, blk)
    coef = orc._svd_dct(orc.to_blocks4(np.array(orc.haar_dwt2(b.frame[: th * 8, : tw * 8, 1])[0]), blk), blk)
    u, s, v = np.linalg.svd(coef)
    enc = orc.DwtDctSvdEncoderOracle(scales=scales, blk=blk, pair_override={1: (u[..., :, 0], v[..., 0, :])})
    enc.read_wm(b.wm)
    assert np.array_equal(enc.encode(b.frame.copy()), ref["marked"])
    nothing = np.full(u[..., :, 0].shape, np.nan, F)
    enc = orc.DwtDctSvdEncoderOracle(scales=scales, blk=blk, pair_override={1: (nothing, nothing)})
    enc.read_wm(b.wm)
    assert np.array_equal(enc.encode(b.frame.copy()), ref["marked"])
    # another pair inside the eigenspaces of the exactly repeated families: rotate LAPACK's first two pairs by the same angle
    u0, v0 = nothing.copy(), nothing.copy()
    exact = np.isin(b.fam, [b.names.index(n) for n in ("axis", "kron")])
    pick = np.zeros(th * tw, bool)
    pick[: len(b.fam)] = exact
    pick = pick.reshape(th, tw)
    c, sn = np.cos(0.7), np.sin(0.7)
    u0[pick] = (c * u[..., :, 0] + sn * u[..., :, 1])[pick]
    v0[pick] = (c * v[..., 0, :] + sn * v[..., 1, :])[pick]
    enc = orc.DwtDctSvdEncoderOracle(scales=scales, blk=blk, pair_override={1: (u0, v0)})
    enc.read_wm(b.wm)
    other = enc.encode(b.frame.copy())
    assert not np.array_equal(other, ref["marked"])
    changed = np.abs(other - ref["marked"])[: th * 8, : tw * 8, 1].reshape(th, 8, tw, 8).max((1, 3)) > 1e-3
    assert changed[pick].mean() > 0.9 and not changed[~pick].any()                 # a different marking, only where handed
    assert not sr.check(b, scales, ref, other, "oracle+pair")                       # ... and as admitted as LAPACK's


def _replay_marked_frame(b, scales, slow_path=None):
    """The float32 replay's marked LL blocks written into a copy of the frame's LL (blk 4), as the frame the check reads."""
    out = b.frame.copy()
    n = len(b.bits)
    info = {}
    for ch in range(3):
        if scales[ch] > 0:
            B = sr.haar_ll(b.frame, ch, 4)[:n]
            r = rp.svd4_top(B) if slow_path is None else rp.svd4_top(B, slow_path=slow_path)
            Bm = rp.marked_ll(B, r["s0"], r["w"], r["v"], b.bits, scales[ch])
            for c in range(n):
                i, j = divmod(c, sr.TILES_PER_ROW)
                out[i * 8:(i + 1) * 8, j * 8:(j + 1) * 8, ch] += np.kron(F(0.5) * (Bm[c] - B[c]), np.ones((2, 2), F))
            info[ch] = r
    return out, info


def test_svd4_top_float32_replay_stays_inside_the_admitted_set():
    """svd4_top / svd_update line by line in float32 (gram, the ten cofactors, the column choice, normalisation, the trigger and
    the Jacobi slow path, w = B v, s0 = |w|, the floor division and the rank-one change) over every family, three channel sets:
    the device tolerances (10 x the reference level per family, floor 10 x the control family's, |sigma_top - s0'| <= scale / 64).
    Before the slow path existed this failed on the axis, kron, rotated-exact, near-gamma and below families with d up to 10."""
    b = sr.build(4)
    for scales in sr.SCALE_SETS:
        ref = sr.reference(4, scales)
        marked, info = _replay_marked_frame(b, scales)
        bad = sr.check(b, scales, ref, marked, "replay")
        assert not bad, "\n".join(bad)
        for ch, r in info.items():
            slow = r["slow"]
            for name in ("control", "threshold"):
                assert not slow[b.fam == b.names.index(name)].any()                # resolved blocks never take the slow path
            for name in ("axis", "kron", "rotated-exact"):
                assert slow[b.fam == b.names.index(name)].all()
            assert r["sweeps"].max() <= (rp.constants()["jcap"] or 0) - 2, r["sweeps"].max()   # the cap is never what ends the loop
            print(f"replay blk4 scales={scales} ch{ch}: slow path on {int(slow.sum())} of {slow.size} tiles, sweeps max {r['sweeps'].max()}, "
                  f"mean {r['sweeps'][slow].mean():.2f}")


def test_repeated_top_values_lose_watermark_bits_without_the_slow_path_and_keep_them_with_it():
    """The payload side of the defect, on the replay.  The worked case -- two 4x4-pixel squares of 23 on zero, placed diagonally in the
    8x8 tile: LL = 46 [[J, 0], [0, J]], singular values 92, 92, 0, 0, bits 0 and 1, scale 15 -- is marked to 93.75 / 101.25 by the
    reference and read back as [0, 1], and so it is by the replay with the slow path.  Without it (the solver as it was) the
    adjugate of a repeated top value is rounding noise: where the Laguerre eigenvalue is exact every cofactor is 0 and the vector
    is e0; where it is an ulp off the column is (by luck of the structure) still usable; where the Gram matrix carries its own
    rounding the column is arbitrary.  Over the exactly repeated families that loses watermark bits the reference keeps."""
    tile = np.zeros((8, 8), F)
    tile[:4, :4] = tile[4:, 4:] = 23
    frame = np.zeros((8, 16, 3), F)
    frame[:, :8, 1] = frame[:, 8:, 1] = tile
    B = sr.haar_ll(frame, 1, 4)
    assert np.array_equal(B[0], 46 * np.kron(np.eye(2), np.ones((2, 2)))) and np.array_equal(B[0], B[1])
    bits = np.array([0, 1], np.uint8)
    enc = orc.DwtDctSvdEncoderOracle()
    enc.read_wm(bits[None])
    ref = enc.encode(frame.copy())
    assert np.array_equal(orc.DwtDctSvdDecoderOracle().decode(ref)[0, :2], [0, 1])
    top = lambda Bm: np.linalg.svd(Bm.astype(np.float64), compute_uv=False)[:, 0]      # noqa: E731
    assert np.allclose(top(sr.haar_ll(ref, 1, 4)), [93.75, 101.25], atol=1e-3)
    new = rp.svd4_top(B, slow_path=True)
    assert new["slow"].all() and np.allclose(new["s0"], 92, atol=1e-4)
    t_new = top(rp.marked_ll(B, new["s0"], new["w"], new["v"], bits, 15.0))
    assert np.allclose(t_new, [93.75, 101.25], atol=1e-3) and np.array_equal(np.mod(t_new, 15) > 7.5, [False, True])
    # the families: bits read from the replay's marked blocks (float64 read-out) against the bits written
    b = sr.build(4)
    n = len(b.bits)
    Bf = sr.haar_ll(b.frame, 1, 4)[:n]
    exact = np.isin(b.fam, [b.names.index(name) for name in ("axis", "kron", "rotated-exact")])
    kept_by_reference = sr.decode_decision(sr.haar_ll(sr.reference(4, (0.0, 15.0, 0.0))["marked"], 1, 4)[:n], 15.0)[0] == b.bits
    assert kept_by_reference[exact].all()
    lost = {}
    for slow in (False, True):
        r = rp.svd4_top(Bf, slow_path=slow)
        read = sr.decode_decision(rp.marked_ll(Bf, r["s0"], r["w"], r["v"], b.bits, 15.0), 15.0)[0]
        lost[slow] = int((read != b.bits)[exact].sum())
    print(f"exactly repeated tiles {int(exact.sum())}: bits lost without the slow path {lost[False]}, with it {lost[True]}")
    assert lost[False] >= 5 and lost[True] == 0


def test_fixture_blocks_stay_on_the_fast_path():
    """The slow path is taken only below the trigger, and no block of a committed svd_*.npz frame (all three channels) or of
    the synthetic frames the GPU tests mark comes within a factor 16 of it: their marked bytes are what they were."""
    import os
    from conftest import GOLDEN, svd_golden_cases
    frames = [np.load(os.path.join(GOLDEN, c + ".npz"))["frame"] for c in svd_golden_cases()]
    frames += [orc.synthetic_frame(240, 320, 1001), orc.synthetic_frame(360, 640, 2000)]
    noise = float(rp.constants()["noise"] or np.inf)                       # no trigger in the source: nothing keeps a block off the fallback
    lowest = np.inf
    for frame in frames:
        yuv = orc.bgr2yuv_f32(frame.astype(F))
        for ch in range(3):
            r = rp.svd4_top(sr.haar_ll(yuv, ch, 4))
            assert not r["slow"].any()
            pos = r["lam"] > 0
            lowest = min(lowest, float((r["best"][pos] / r["lam"][pos].astype(np.float64) ** 3).min(initial=np.inf)))
    print(f"lowest best / lam^3 over the fixture blocks: {lowest:.3e} (trigger {noise:.3e})")
    assert lowest >= 16 * noise


@pytest.mark.parametrize("blk", [4, 8])
def test_u8_tiles_have_their_spectra_and_a_usable_rounding_level(blk):
    """The u8 RGB tiles of the GPU test (u8_tiles asserts each tile's LL structure, cluster size and remainder while generating):
    the oracle marks them, reads every bit back, and the u8 rounding level of the sorted singular values, doubled, stays below a
    quarter step -- otherwise the device comparison would prove nothing.  blk 4: the float32 replay of svd4_top leaves the
    singular values {s0', sigma_1, ...} to float32 accuracy on every tile, all through the slow path."""
    t = sr.u8_tiles(blk)
    scale = sr.U8_SCALE[blk]
    n = len(t.bits)
    assert t.frame.dtype == np.uint8 and t.frame.shape[0] % 16 == 0 and t.frame.shape[1] % 16 == 0 and t.tags.count("multi") >= 24
    for r0 in range(0, t.frame.shape[0], 2):
        assert np.array_equal(t.frame[r0], t.frame[r0 + 1]) and np.array_equal(t.frame[:, r0::2][:, :1], t.frame[:, r0 + 1::2][:, :1])      # uniform over 2x2
    enc = orc.DwtDctSvdEncoderOracle(scales=(0, scale, 0), blk=blk)
    enc.read_wm(t.wm)
    ref = orc.mark_frame(t.frame, enc)
    assert enc.debug_ch[1]["gap"].reshape(-1)[:n].min() >= 1 - 2.5e-5 and 0 < ref.min() and ref.max() < 255
    level = float(sr.spectrum_error(t, ref).max())
    print(f"oracle blk{blk} u8 tiles={n} scale={scale}: spectrum error level {level:.3f}, device bound {2 * level:.3f}, scale / 4 = {scale / 4}")
    assert 2 * level < scale / 4
    assert np.array_equal(orc.check_frame(ref, orc.DwtDctSvdDecoderOracle(scales=(0, scale, 0), blk=blk))[0, :n], t.bits)
    if blk == 4:
        B = sr.u8_ll(t.frame, 4)[:n]
        r = rp.svd4_top(B)
        got = np.linalg.svd(rp.marked_ll(B, r["s0"], r["w"], r["v"], t.bits, scale).astype(np.float64), compute_uv=False)
        want = t.sigma.copy()
        want[:, 0] = sr.s_new(np.floor(t.sigma[:, 0] / scale), t.bits, scale)
        assert r["slow"].all() and np.abs(np.sort(got, 1) - np.sort(want, 1)).max() <= 64 * 2.0 ** -24 * t.sigma[:, 0].max()


def test_u8_luma_tiles_and_down_marked_tiles():
    """The other two u8 tile sets of the GPU test.  Luma tiles (u8_y_tiles asserts LL = a P exactly while generating): the svd4_top
    replay takes a coordinate vector (all through the slow path, no rotation) and leaves {s0', a, a, a} to float32 accuracy; the
    oracle's own u8 frame does not (its pair is not axis aligned and the black pixels clip), which is why the GPU test reasons its
    bound for these tiles.  Down-marked tiles: the marked spectrum keeps three top values close together, and the float32 replay
    of the verify's loose solve (gram_top_eigenvalue at kTolLoose, kCapLoose) against the stand-alone read-out's tight one on the
    oracle's marked frame: it ends at its cap, the two agree to the figure printed, well inside the 4.4e-5 relative of the kernel
    comment, and decide alike unless the top value is that close to a threshold."""
    from test_kernel_arithmetic import _svd_gram, _svd_top_eigenvalue
    for blk in (4, 8):
        t = sr.u8_y_tiles(blk)
        scale = sr.U8_SCALE[blk]
        enc = orc.DwtDctSvdEncoderOracle(scales=(scale, 0, 0), blk=blk)
        enc.read_wm(t.wm)
        level = float(sr.spectrum_error(t, orc.mark_frame(t.frame, enc), 0).max())
        print(f"oracle blk{blk} u8 luma tiles={len(t.bits)} scale={scale}: spectrum error level {level:.3f} (a quarter step is {scale / 4})")
        if blk == 4:
            B = sr.u8_ll(t.frame, 4, 0)[: len(t.bits)]
            r = rp.svd4_top(B)
            assert r["slow"].all() and r["sweeps"].max() == 1 and (np.abs(r["v"]).max(1) == 1).all()
            got = np.linalg.svd(rp.marked_ll(B, r["s0"], r["w"], r["v"], t.bits, scale).astype(np.float64), compute_uv=False)
            want = t.sigma.copy()
            want[:, 0] = sr.s_new(np.floor(t.sigma[:, 0] / scale), t.bits, scale)
            assert np.abs(np.sort(got, 1) - np.sort(want, 1)).max() <= 64 * 2.0 ** -24 * t.sigma[:, 0].max()
    t = sr.u8_tiles(4, down=True)
    scale = sr.U8_SCALE[4]
    enc = orc.DwtDctSvdEncoderOracle(scales=(0, scale, 0), blk=4)
    enc.read_wm(t.wm)
    B = sr.u8_ll(orc.mark_frame(t.frame, enc), 4)[: len(t.bits)]
    s64 = np.linalg.svd(B.astype(np.float64), compute_uv=False)
    assert ((s64[:, 0] - s64[:, 2]) / s64[:, 0]).max() < 0.02                 # three top values within 2 %
    k = rp.constants()
    import re
    tol_l = F(float(re.search(r"kTolLoose = ([0-9.eE+-]+)f", rp.SRC).group(1)))
    cap_l = int(re.search(r"kCapLoose = (\d+)", rp.SRC).group(1))
    G = _svd_gram(B)
    tight, _ = _svd_top_eigenvalue(G, k["tol"], k["cap"])
    loose, it = _svd_top_eigenvalue(G, tol_l, cap_l)
    diff = np.abs(np.sqrt(tight) - np.sqrt(loose))
    print(f"down-marked tiles={len(t.bits)}: loose solve iterations max {it.max()} (cap {cap_l}); |s0 loose - s0 tight| max {diff.max():.2e} "
          f"({(diff / s64[:, 0]).max():.1e} relative)")
    assert (diff / s64[:, 0]).max() <= 4.4e-5
