"""CPU: the statement of tests/_ambiguous.py held against the reference itself.

In a block whose C21 is float rounding noise the reference's result is one of three (np.sign = +1 / -1 / 0, dct_encoder.py:33-35).
Here every stored vector -- the reference's own modules over the oracle's primitives (tests/golden/, compared under "legacy"
promotion like test_gpu_parity.py does) and over independent scipy / NumPy primitives (tests/golden_scipy/, "nep50") -- is checked
to stay inside that statement in EVERY ambiguous block, at the project's pixel budget (<= 1 LSB on <= 1e-5 of the samples, floor
1; measured: 0 samples off in all cases).  That is the yardstick for test_gpu_ambiguous.py, which holds the HIP kernels to the one
candidate their own C21 names.  Then the properties of the candidates and of the oracle's forced sign."""
import os

import numpy as np
import pytest

import _ambiguous as ab
import offmark_oracle as orc
from conftest import GOLDEN, ROOT, golden_cases

GOLDEN_SCIPY = os.path.join(ROOT, "tests", "golden_scipy")
CROPS = ["frame63_crop0_L8_k0_a20", "frame63_crop1_L8_k0_a20", "frame63_crop_qr_k0_a20"]


def scipy_cases():
    return sorted(f[:-4] for f in os.listdir(GOLDEN_SCIPY) if f.endswith(".npz") and not f.startswith("svd_"))


@pytest.mark.parametrize("fixtures,promotion,case", [("golden_scipy", "nep50", c) for c in scipy_cases()] +
                         [("golden", "legacy", c) for c in golden_cases()])
def test_every_ambiguous_block_of_a_vector_is_one_of_the_three_candidates(fixtures, promotion, case):
    g = np.load(os.path.join(ROOT, "tests", fixtures, case + ".npz"))
    frame, alpha = g["frame"], float(g["alpha"])
    H, W, _ = frame.shape
    c = ab.candidates(frame, g["wm"], alpha, promotion)
    signs = ab.best_signs(g["marked"], c.frames, c.amb)
    zero = c.amb & (signs == 0)
    px = ab.block_pixels(zero, H, W)
    assert np.array_equal(g["marked"][px], c.frames[2][px])              # "0" only where the vector's block equals it
    want = ab.expected_from_signs(c.frames, c.amb, np.where(c.amb, signs, 1.0))
    bad = ab.assert_frame(g["marked"], want, ab.block_pixels(c.amb, H, W), what=case)
    n = ab.sign_counts(c.amb, signs)
    print(f"{fixtures}/{case}: {int(c.amb.sum())} of {c.amb.size} blocks ambiguous, nearest candidate + / - / 0 = {n[0]} / {n[1]} / {n[2]}; "
          f"{bad} of {int(c.amb.sum()) * 192} samples off")


@pytest.fixture(scope="module", params=CROPS)
def crop(request):
    g = np.load(os.path.join(GOLDEN, request.param + ".npz"))
    return g["frame"], g["wm"], float(g["alpha"]), ab.candidates(g["frame"], g["wm"], float(g["alpha"]))


def test_candidates_differ_exactly_where_the_statement_says(crop):
    frame, wm, alpha, c = crop
    H, W, _ = frame.shape
    plus, minus, zero = c.frames
    rows, cols = c.amb.shape
    bit1 = wm.reshape(-1)[: rows * cols].reshape(rows, cols) != 0
    assert c.amb.any() and (c.amb & bit1).any() and (c.amb & ~bit1).any()
    # outside the ambiguous blocks: the oracle's ordinary result, in all three
    enc = orc.DctEncoderOracle(alpha=alpha)
    enc.read_wm(wm)
    ordinary = orc.mark_frame(frame, enc)
    out = ~ab.block_pixels(c.amb, H, W)
    for f in c.frames:
        assert np.array_equal(f[out], ordinary[out])
    # bit 0: q == 0, the three coincide; bit 1: q == step, +step and -step patterns differ in every such block
    same = ab.block_pixels(c.amb & ~bit1, H, W)
    assert np.array_equal(plus[same], minus[same]) and np.array_equal(plus[same], zero[same])

    def differ(a, b):
        return (a[: rows * 8, : cols * 8] != b[: rows * 8, : cols * 8]).reshape(rows, 8, cols, 8, 3).any(axis=(1, 3, 4))
    assert differ(plus, minus)[c.amb & bit1].all()
    assert differ(plus, zero)[c.amb & bit1].all() and differ(minus, zero)[c.amb & bit1].all()
    print(f"{int((c.amb & bit1).sum())} ambiguous bit-1 blocks of {int(c.amb.sum())} ambiguous, all with + != -")
    # the ordinary result is the candidate of the oracle's own sign
    assert np.array_equal(ab.expected_from_signs(c.frames, c.amb, np.sign(c.debug["c21_pre"])), ordinary)


def test_candidates_equal_full_oracle_passes_with_the_sign_forced(crop):
    frame, wm, alpha, c = crop
    for s, cand in zip((1.0, -1.0, 0.0), c.frames):
        enc = orc.DctEncoderOracle(alpha=alpha, sign_override=np.where(c.amb, s, np.nan))
        enc.read_wm(wm)
        assert np.array_equal(orc.mark_frame(frame, enc), cand)
    # a mixed choice: expected_from_signs against one full pass
    rng = np.random.default_rng(5)
    signs = rng.integers(-1, 2, c.amb.shape).astype(np.float64)
    enc = orc.DctEncoderOracle(alpha=alpha, sign_override=np.where(c.amb, signs, np.nan))
    enc.read_wm(wm)
    assert np.array_equal(orc.mark_frame(frame, enc), ab.expected_from_signs(c.frames, c.amb, signs))


@pytest.mark.parametrize("promotion", ["legacy", "nep50"])
def test_no_override_is_the_oracle_of_before_and_loop_equals_vec_under_one(promotion):
    g = np.load(os.path.join(GOLDEN, "syn_30x44_L8_k0_a20.npz"))
    nat = np.load(os.path.join(GOLDEN, CROPS[0] + ".npz"))
    for frame, wm, alpha in ((g["frame"], g["wm"], float(g["alpha"])), (nat["frame"][:40, 24:80], nat["wm"], float(nat["alpha"]))):
        yuv = orc.bgr2yuv_f32(frame.astype(np.float32))
        rows, cols = yuv.shape[0] // 8, yuv.shape[1] // 8

        def run(form, override):
            enc = orc.DctEncoderOracle(alpha=alpha, form=form, promotion=promotion, sign_override=override)
            enc.read_wm(wm)
            return enc.encode(yuv.copy()), enc.debug

        plain, dbg = run("vec", None)
        # all-NaN override == no override == np.sign of the coefficient given explicitly
        assert np.array_equal(run("vec", np.full((rows, cols), np.nan))[0], plain)
        assert np.array_equal(run("vec", np.sign(dbg["c21_pre"]))[0], plain)
        assert np.array_equal(run("loop", None)[0], plain)
        rng = np.random.default_rng(11)
        override = rng.choice([-1.0, 0.0, 1.0, np.nan], (rows, cols))
        v, dv = run("vec", override)
        l, dl = run("loop", override)
        assert np.array_equal(v, l) and np.array_equal(dv["c21_post"], dl["c21_post"])
        forced = ~np.isnan(override)
        assert np.array_equal(np.sign(dv["c21_post"][forced & (dv["c21_post"] != 0)]), override[forced & (dv["c21_post"] != 0)])
        assert (dv["c21_post"][override == 0] == 0).all()
        assert not np.array_equal(v, plain)


def test_qim_embed_sign_argument():
    c = np.array([3.0, -3.0, 0.0, 1e-6, -1e-6, 45.0], np.float32)
    step, bits = np.full(6, 20.0), np.array([1, 1, 1, 1, 0, 0])
    ref = orc.qim_embed(c, step, bits)
    assert np.array_equal(ref, np.array([20, -20, 0, 20, -0.0, 40], np.float32))
    assert np.array_equal(orc.qim_embed(c, step, bits, sign=np.nan), ref)
    assert np.array_equal(orc.qim_embed(c, step, bits, sign=-1), np.array([-20, -20, -20, -20, -0.0, -40], np.float32))
    assert np.array_equal(orc.qim_embed(c, step, bits, sign=[np.nan, 1, 1, 0, 1, np.nan]), np.array([20, 20, 20, 0, 0, 40], np.float32))
    with pytest.raises(ValueError):
        orc.qim_embed(c, step, bits, sign=2)
