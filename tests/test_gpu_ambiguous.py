"""GPU: the pixels the DCT mark kernels write INSIDE sign-ambiguous blocks, against the oracle.

Every other pixel comparison of the suite masks out the blocks whose |C21| <= 1e-3 (up to 15 % of natural frames, every block of
R = G = B video), because the reference's np.sign(C21) is float noise there.  The result is still one of three known frames
(tests/_ambiguous.py; held against the reference's own vectors on the CPU by test_ambiguous_statement.py), and the library names
which: ofmk_debug_planes runs the same analyze pass on the same bytes as ofmk_embed_rgb8 / ofmk_embed_detect_rgb8 and reports the
record's C21 as c21_pre, the very float mark_delta consumes.  So here sign(c21_pre) picks the candidate per ambiguous block and
the marked frame is compared with it over the WHOLE frame at the project's pixel budget (<= 1 LSB on <= 1e-5 of the samples,
floor 1).  No best-of-three: a kernel whose mark path disagreed with the C21 it reports fails.

What needs no test of its own: 4:2:0 planes and the one-pass copies calls.  test_gpu_planar.py pins the planar path to the RGB
chain bit for bit; test_gpu_copies.py and test_gpu_planar_copies.py pin the copies kernels to single-copy embeds bit for bit.  The
RGB kernels checked here are the root of all of them."""
import functools
import os

import numpy as np
import pytest

import _ambiguous as ab
import offmark_oracle as orc
from conftest import GOLDEN
from test_gpu_parity import _dump_measured, _log          # noqa: F401  the parity log and the fixture that writes it out

pytestmark = pytest.mark.gpu

P8 = np.array([0, 1, 1, 0, 0, 1, 0, 1])
BITS_FRAC = 1e-4         # the project's block budget for mask threshold flips (test_gpu_parity.py)
CROPS = ["frame63_crop0_L8_k0_a20", "frame63_crop1_L8_k0_a20", "frame63_crop_qr_k0_a20"]
EDGES = ["edge_black_64x64", "edge_gray_64x64", "edge_white_64x64"]


@pytest.fixture(scope="module")
def engines():
    import torch
    from offmark.engine import DctEngine
    torch.cuda.set_device(0)
    return {"auto": DctEngine(), "linear": DctEngine(tile_order="linear"), "xcd": DctEngine(tile_order="xcd")}


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()          # a copy: the shared inputs are read-only


def gray_frame(H, W):
    """R = G = B: U is rounding noise around 0.5, every block is ambiguous."""
    return np.repeat(orc.synthetic_frame(H, W, 1001)[:, :, 1:2], 3, axis=2)


@functools.lru_cache(maxsize=None)
def case_input(case):
    """-> (frame, wm [1, N], alpha, Candidates): computed once per case and shared, never written to."""
    if case.startswith("gray_"):
        H, W = (int(v) for v in case[5:].split("x"))
        frame, wm, alpha = gray_frame(H, W), orc.shuffle_generate(P8, (1, H * W // 64), 0), 20.0
    else:
        g = np.load(os.path.join(GOLDEN, case + ".npz"))
        frame, wm, alpha = g["frame"], g["wm"], float(g["alpha"])
    c = ab.candidates(frame, wm, alpha)
    for a in (frame, wm, c.amb) + c.frames:
        a.setflags(write=False)
    return frame, wm, alpha, c


@pytest.mark.parametrize("case", CROPS + EDGES + ["gray_240x320"])
def test_marked_pixels_follow_the_sign_of_the_kernels_own_c21(engines, case):
    frame, wm, alpha, c = case_input(case)
    L = 8
    assert c.amb.any()
    if case in EDGES or case.startswith("gray_"):
        assert c.amb.all()
    first = None
    for order, eng in engines.items():
        c21 = eng.debug_planes(cuda(frame), alpha=alpha, wm=wm)["c21_pre"]
        marked = eng.embed(cuda(frame[None]), wm, alpha=alpha)[0].cpu().numpy()
        fused = eng.embed_detect(cuda(frame[None]), wm, L=L, alpha=alpha)[0][0].cpu().numpy()
        assert np.array_equal(marked, fused), order                     # ofmk_embed_rgb8 == ofmk_embed_detect_rgb8, byte for byte
        n = ab.assert_marked_by_own_sign(marked, c, c21, what=f"{case} / {order}", log=_log)
        if first is None:
            first = marked
            print(f"{case}: {int(c.amb.sum())} of {c.amb.size} blocks ambiguous; the kernel's C21 is + / - / 0 in {n[0]} / {n[1]} / {n[2]}")
        assert np.array_equal(marked, first), order                     # tile orders write the same bytes


def test_batch_with_frame_index_and_watermark_rows(engines):
    """Three frames in one call, a two-row watermark table and wm_row = [1, 0, 1]: the frame index and the watermark-row paths of
    the mark kernels get the same pixel check, ambiguous blocks included."""
    eng = engines["auto"]
    frames = np.stack([case_input(CROPS[0])[0], case_input(CROPS[1])[0], gray_frame(128, 128)])
    N = 128 * 128 // 64
    wm = np.concatenate([orc.shuffle_generate(P8, (1, N), 0), orc.shuffle_generate(1 - P8, (1, N), 3)])
    rows = np.array([1, 0, 1], np.int32)
    assert (wm[0] != wm[1]).any()
    marked = eng.embed(cuda(frames), wm, alpha=20, wm_row=rows).cpu().numpy()
    fused = eng.embed_detect(cuda(frames), wm, L=8, alpha=20, wm_row=rows)[0].cpu().numpy()
    assert np.array_equal(marked, fused)
    for k in range(3):
        c = ab.candidates(frames[k], wm[rows[k]][None], 20.0)
        assert c.amb.any()
        c21 = eng.debug_planes(cuda(frames[k]), alpha=20, wm=wm[rows[k]][None])["c21_pre"]
        n = ab.assert_marked_by_own_sign(marked[k], c, c21, what=f"frame {k}", log=_log)
        # the other row's watermark would not pass: the check is sensitive to the row
        other = ab.candidates(frames[k], wm[1 - rows[k]][None], 20.0)
        assert not np.array_equal(ab.expected_from_signs(other.frames, other.amb, np.sign(c21)), marked[k])
        print(f"frame {k} (wm row {rows[k]}): {int(c.amb.sum())} of {c.amb.size} blocks ambiguous; + / - / 0 = {n[0]} / {n[1]} / {n[2]}")


@pytest.mark.parametrize("case", [CROPS[0], "gray_240x320"])
def test_float_plugin_boundary_inside_ambiguous_blocks(case):
    """DctEncoder.encode(yuv) (ofmk_encode_yuv32f) on float32 YUV: the U plane against the oracle with the sign of the
    library's own C21 (debug_planes of the float frame) forced in the ambiguous blocks, within the 2e-3 of
    test_yuv_plugin_boundary, over every block (budget: the samples of the project's share of threshold-flip blocks)."""
    from offmark.embed.dct_encoder import DctEncoder
    frame, wm, alpha, _ = case_input(case)
    yuv = orc.bgr2yuv_f32(frame.astype(np.float32))
    nblk = (yuv.shape[0] // 8) * (yuv.shape[1] // 8)
    plain = orc.DctEncoderOracle(alpha=alpha)
    plain.read_wm(wm)
    plain.encode(yuv.copy())
    amb = np.abs(plain.debug["c21_pre"]) <= ab.C21_TOL
    assert amb.any() and (2 * alpha * plain.debug["mask"][amb] > 4 * ab.C21_TOL).all()
    enc = DctEncoder(alpha=alpha)
    enc.read_wm(wm)
    c21 = enc.engine.debug_planes(cuda(yuv), alpha=alpha, wm=wm)["c21_pre"]
    signs = np.sign(c21.astype(np.float64))
    forced = orc.DctEncoderOracle(alpha=alpha, sign_override=np.where(amb, signs, np.nan))
    forced.read_wm(wm)
    ref = forced.encode(yuv.copy())
    got = enc.encode(yuv.copy())
    assert np.array_equal(got[:, :, 0], yuv[:, :, 0]) and np.array_equal(got[:, :, 2], yuv[:, :, 2])
    far = np.abs(got[:, :, 1] - ref[:, :, 1]) > 2e-3
    _log("yuv_u_ambiguous", far.sum(), far.size)
    n = ab.sign_counts(amb, signs)
    for name, k in zip(("plus", "minus", "zero"), n):
        _log("ambiguous_sign_" + name, k, int(amb.sum()))
    print(f"{case}: {int(amb.sum())} of {nblk} blocks ambiguous; + / - / 0 = {n[0]} / {n[1]} / {n[2]}; {int(far.sum())} U samples beyond 2e-3, "
          f"max |dU| = {np.abs(got[:, :, 1] - ref[:, :, 1]).max():.3g}")
    assert far.sum() <= 64 * ab.budget(nblk, BITS_FRAC)
