"""GPU: every leaf and both sides of every threshold of the DCT codec's perceptual masks, on every kernel that inlines them.

texture_code() (csrc/common.hiph) is the reference's texture_mask decision tree, branch-free, with four float32 threshold
constants; luminance_value() is its luminance tree.  block_features() inlines the first into every DCT frame kernel (analyze,
fused mark, finalize, the 4:2:0 pair, both copies kernels, both resync searches), each a separate instantiation.  The fixtures the
suite had before reach neither the big arm's ratio clauses nor the neighbourhood of most thresholds
(profiles/mask_leaves_tests.txt), and compare the masks at a budget of 1e-4 flipped blocks that was never used.

Here the inputs are the two "zoo" frames of tests/_mask_leaves.py (tests/golden/mask_leaves_zoo.npy; one frame whose mean clamps
at 90, one above): at least 8 tau-stable blocks on every feasible leaf, at least 4 on each side of each of the 13 texture
comparisons and of 15 / 25 / the frame mean within 1e-3 relative, and a few blocks that are undecidable on purpose.  tau is ten
times the oracle's own float32 level; a tau-stable block's leaf does not depend on rounding, so the budget for flipped blocks is
ZERO.  An unstable block must take a value of its admitted set, and everything downstream of it is compared with the oracle
rebuilt under the value the device chose.  No block is sign-ambiguous (|C21| >= 1): nothing is masked out."""
import numpy as np
import pytest

import _ambiguous as ab
import _mask_leaves as ml
import offmark_oracle as orc

pytestmark = pytest.mark.gpu

P8 = np.array([0, 1, 1, 0, 0, 1, 0, 1])
N = 256                                                      # blocks per zoo frame
WM = orc.shuffle_generate(P8, (1, N), 0)
LAYOUTS = ("i420", "nv12")
_REPORT = []


@pytest.fixture(scope="module")
def eng():
    import torch
    from offmark.engine import DctEngine
    torch.cuda.set_device(0)
    return DctEngine()


@pytest.fixture(scope="module")
def zoo():
    return ml.stored_zoo()


@pytest.fixture(scope="module", autouse=True)
def _dump_report():
    yield
    ml.write_report("mask_leaves_device.txt", _REPORT)


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()               # a copy: the shared inputs are read-only


def report(line):
    _REPORT.append(line)


def check_planes(d, fl, alpha, tau, what):
    """debug_planes of a labelled frame: Y DC and C21 within the file-wide 1e-3, tex / lum by ml.device_choice (zero budget on
    tau-stable blocks, the admitted set elsewhere), step = alpha * tex * lum of the values the device itself chose.
    -> (the device's mask choice for oracle_mark / oracle_read, the largest |read-back eh - float64 eh| over stable ramp blocks)."""
    assert np.abs(d["y_dc"] - fl.ft.ydc).max() <= 1e-3 and np.abs(d["c21_pre"] - fl.ft.c21).max() <= 1e-3, what
    assert np.abs(d["y_dc"] - fl.ft.f64[0]).max() < tau, what             # the device's A00 against the float64 one: inside tau, as the
    #                                                                       luminance tree's zero budget needs (m = A00 / 8 against tau / 8)
    choice = ml.device_choice(fl, d["tex"], d["lum"], tau, what)
    assert np.abs(d["step"] - alpha * (d["tex"] * d["lum"])).max() <= 1e-12 * alpha * 4, what
    ramp = (np.isin(fl.tex.leaf, (ml.T_BIG_RAMP, ml.T_SMALL_RAMP)).reshape(-1) & fl.tex_stab.stable).reshape(fl.m.shape)
    eh_back = 290 + 1510 * (d["tex"][ramp] - 1) / 1.25
    return choice, float(np.abs(eh_back - fl.ft.f64[2][ramp]).max())


@pytest.mark.parametrize("k", [0, 1], ids=["clamped", "unclamped"])
def test_masks_on_every_leaf_and_threshold_side(eng, zoo, k):
    frame, fl = zoo.frames[k], zoo.labels[k]
    d = eng.debug_planes(cuda(frame), alpha=20.0, wm=WM)
    choice, level = check_planes(d, fl, 20.0, zoo.tau, f"zoo frame {k}")
    # the device's eh, read back from the ramp values: its distance from the float64 eh is the device's level; the zero budget
    # stands on it being inside tau
    report(f"zoo frame {k} u8: largest |device eh (read back from the ramp) - float64 eh| = {level:.3g}; oracle level {zoo.level:.3g}, tau {zoo.tau:.3g}")
    assert level < zoo.tau
    unstable = ml.unstable_blocks(fl)
    dev_mask = d["tex"] * d["lum"]
    _, dbg = ml.oracle_mark(frame, WM, 20.0, choice)
    assert np.abs(dev_mask - dbg["mask"]).max() <= 2e-5               # stable: 2e-6 each; unstable: the nearest admitted value
    assert np.abs(d["c21_post"] - dbg["c21_post"]).max() <= 2e-3
    report(f"zoo frame {k}: {int(unstable.sum())} unstable blocks, the device agrees with the oracle's own choice on "
           f"{int((np.abs(dev_mask - fl.tex.value * fl.lum_value) <= 2e-5)[unstable].sum())} of them")
    # the float-YUV plugin boundary reads the same trees (ofmk_debug_planes on float32 YUV)
    dy = eng.debug_planes(cuda(orc.bgr2yuv_f32(frame.astype(np.float32))), alpha=20.0, wm=WM)
    _, level_y = check_planes(dy, fl, 20.0, zoo.tau, f"zoo frame {k} (float YUV)")
    assert level_y < zoo.tau


@pytest.mark.parametrize("k", [0, 1], ids=["clamped", "unclamped"])
def test_marked_frames_against_the_oracle_under_the_devices_own_choice(eng, zoo, k):
    from offmark.embed.dct_encoder import DctEncoder
    frame, fl = zoo.frames[k], zoo.labels[k]
    for alpha in (20.0, 7.3):
        d = eng.debug_planes(cuda(frame), alpha=alpha, wm=WM)
        choice, _ = check_planes(d, fl, alpha, zoo.tau, f"zoo frame {k}")
        want, _ = ml.oracle_mark(frame, WM, alpha, choice)
        marked = eng.embed(cuda(frame[None]), WM, alpha=alpha)[0].cpu().numpy()
        fused = eng.embed_detect(cuda(frame[None]), WM, L=8, alpha=alpha)[0][0].cpu().numpy()
        assert np.array_equal(marked, fused)
        bad = ab.assert_frame(marked, want, None, what=f"zoo frame {k}, alpha {alpha}")        # the project's pixel budget, whole frame
        report(f"zoo frame {k} alpha {alpha}: {bad} of {marked.size} marked samples differ from the oracle")
        # float-YUV boundary (ofmk_encode_yuv32f): U within 2e-3 of the oracle under the device's choice, every sample
        yuv = orc.bgr2yuv_f32(frame.astype(np.float32))
        enc = DctEncoder(alpha=alpha)
        enc.read_wm(WM)
        dy = enc.engine.debug_planes(cuda(yuv), alpha=alpha, wm=WM)
        choice_y, _ = check_planes(dy, fl, alpha, zoo.tau, f"zoo frame {k} (float YUV)")
        ref, _ = ml.oracle_encode_yuv(yuv.copy(), WM, alpha, choice_y)
        got = enc.encode(yuv.copy())
        assert np.array_equal(got[:, :, 0], yuv[:, :, 0]) and np.array_equal(got[:, :, 2], yuv[:, :, 2])
        far = np.abs(got[:, :, 1] - ref[:, :, 1]) > 2e-3
        report(f"zoo frame {k} alpha {alpha}: float U max |d| = {np.abs(got[:, :, 1] - ref[:, :, 1]).max():.3g}, {int(far.sum())} samples beyond 2e-3")
        assert far.sum() == 0


def _readable(x):
    return np.abs(np.abs(x - np.floor(x)) - 0.5) > 1e-4         # test_gpu_sweeps.py's rule


@pytest.mark.parametrize("k", [0, 1], ids=["clamped", "unclamped"])
def test_read_out_of_the_oracle_marked_zoo(eng, zoo, k):
    """detect (want_bits), detect_soft's signs and the 4:2:0 read-out on the oracle-marked frame: the oracle's bits on every block
    that is tau-stable on the decode side and readable (zero budget); and for EVERY block the bit of the float64 quotient of the
    device's own C21 and step (test_fast_readout_equals_float64_for_every_block's check), at alpha 20 and 0.05."""
    marked, _ = ml.oracle_mark(zoo.frames[k], WM, 20.0)
    fl = ml.label_frame(marked, zoo.tau)
    dev = cuda(marked[None])
    for alpha in (20.0, 0.05):
        d = eng.debug_planes(dev[0], alpha=alpha)
        choice, _ = check_planes(d, fl, alpha, zoo.tau, f"marked zoo frame {k}")
        bits_o, x = ml.oracle_read(marked, alpha)
        hold = _readable(x) & ~ml.unstable_blocks(fl).reshape(-1)
        counts, bits = eng.detect(dev, 8, alpha=alpha, want_bits=True)
        bits = bits[0].cpu().numpy()
        assert np.array_equal(bits[hold], bits_o[hold].astype(np.uint8)), (alpha, int((bits != bits_o)[hold].sum()))
        soft = eng.detect_soft(dev, N, alpha=alpha)[0].cpu().numpy()           # L = N: one block per position, sign = bit
        assert np.array_equal((soft > 0)[hold], bits_o[hold] == 1)
        xd = d["c21_pre"].astype(np.float64).reshape(-1) / d["step"].reshape(-1)
        want = (np.around(xd) % 2 == 1).astype(np.uint8)
        assert np.array_equal(bits, want), (alpha, int((bits != want).sum()))
        assert np.array_equal(counts[0].cpu().numpy(), want.reshape(-1, 8).sum(axis=0))
        # unstable blocks too: the oracle's read-out under the device's own mask choice
        bits_c, xc = ml.oracle_read(marked, alpha, choice)
        rd = _readable(xc)
        assert np.array_equal(bits[rd], bits_c[rd].astype(np.uint8))
        report(f"marked zoo frame {k} alpha {alpha}: {int(hold.sum())} of {N} blocks stable and readable, {int(rd.sum())} readable under the device's choice")
    for layout in LAYOUTS:
        planes = orc.pack_yuv420(*orc.rgb_to_yuv420(marked), layout)
        seen = orc.yuv420_to_rgb(*orc.unpack_yuv420(planes, 128, 128, layout))        # what a reader of the planes sees
        fls = ml.label_frame(seen, zoo.tau)
        bits_o, x = ml.oracle_read(seen, 20.0)
        hold = _readable(x) & ~ml.unstable_blocks(fls).reshape(-1)
        _, bits = eng.detect_yuv420(cuda(planes[None]), 128, 128, 8, alpha=20.0, want_bits=True, layout=layout)
        bits = bits[0].cpu().numpy()
        assert np.array_equal(bits[hold], bits_o[hold].astype(np.uint8)), layout
        soft = eng.detect_soft_yuv420(cuda(planes[None]), 128, 128, N, alpha=20.0, layout=layout)[0].cpu().numpy()
        assert np.array_equal((soft > 0)[hold], bits_o[hold] == 1), layout


def _planes(zoo, layout):
    return np.stack([orc.pack_yuv420(*orc.rgb_to_yuv420(f), layout) for f in zoo.frames])


def test_zoo_through_four_two_zero_still_reaches_every_leaf(zoo):
    """What the planar kernels see (the planes converted back, csrc/planar_kernels.hiph) keeps tau-stable blocks on every
    feasible texture leaf and every luminance leaf: the equalities below are not vacuous for the tree."""
    for f in zoo.frames:
        seen = orc.yuv420_to_rgb(*orc.rgb_to_yuv420(f))
        fl = ml.label_frame(seen, zoo.tau)
        rows = ml.zoo_rows(fl)
        for name in ml.TEX_FEASIBLE:
            assert rows["tex:" + name] >= 4, (name, rows["tex:" + name])
        for i in range(4):
            assert ((fl.lum_leaf.reshape(-1) == i) & fl.lum_stab.stable).sum() >= 4


@pytest.mark.parametrize("layout", LAYOUTS)
def test_planar_kernels_equal_the_rgb_chain_on_the_zoo(eng, zoo, layout):
    import torch
    H = W = 128
    planes = cuda(_planes(zoo, layout))
    wm = np.stack([WM[0], 1 - WM[0]])
    rows = np.array([0, 1], np.int32)
    mid = eng.yuv420_to_rgb(planes, H, W, layout)
    ref_out = eng.rgb_to_yuv420(eng.embed(mid, wm, wm_row=rows), layout)
    ref_counts, ref_bits = eng.detect(eng.yuv420_to_rgb(ref_out, H, W, layout), 8, want_bits=True)
    assert torch.equal(eng.embed_yuv420(planes, H, W, wm, wm_row=rows, layout=layout), ref_out)
    out, counts, bits = eng.embed_detect_yuv420(planes, H, W, wm, 8, wm_row=rows, want_bits=True, layout=layout)
    assert torch.equal(out, ref_out) and torch.equal(counts, ref_counts) and torch.equal(bits, ref_bits)
    c3, b3 = eng.detect_yuv420(ref_out, H, W, 8, want_bits=True, layout=layout)
    assert torch.equal(c3, ref_counts) and torch.equal(b3, ref_bits)


def test_copies_kernels_equal_single_copy_calls_on_the_zoo(eng, zoo):
    import torch
    C, H, W = 3, 128, 128
    frames = cuda(np.stack(zoo.frames))
    wm = np.stack([WM[0], 1 - WM[0], np.roll(WM[0], 3)]).astype(np.uint8)
    rows = cuda(np.array([[0, 1], [1, 2], [2, 0]], np.int32))
    out = eng.embed_copies(frames, wm, rows)
    fused, counts, bits = eng.embed_detect_copies(frames, wm, rows, 8, want_bits=True)
    assert torch.equal(out, fused)
    for c in range(C):
        one, c1, b1 = eng.embed_detect(frames, wm, L=8, wm_row=rows[c], want_bits=True)
        assert torch.equal(out[c], eng.embed(frames, wm, wm_row=rows[c])) and torch.equal(out[c], one), c
        assert torch.equal(counts[c], c1) and torch.equal(bits[c], b1), c
    for layout in LAYOUTS:
        planes = cuda(_planes(zoo, layout))
        outp = eng.embed_copies_yuv420(planes, H, W, wm, rows, layout=layout)
        fusedp, countsp, bitsp = eng.embed_detect_copies_yuv420(planes, H, W, wm, rows, 8, want_bits=True, layout=layout)
        assert torch.equal(outp, fusedp)
        for c in range(C):
            one, c1, b1 = eng.embed_detect_yuv420(planes, H, W, wm, 8, wm_row=rows[c], want_bits=True, layout=layout)
            assert torch.equal(outp[c], one) and torch.equal(countsp[c], c1) and torch.equal(bitsp[c], b1), (layout, c)


def test_resync_searches_equal_the_soft_read_out_of_the_shifted_crops(eng, zoo):
    """sync_scores and sync_scores_yuv420 on the oracle-marked zoo: integer for integer the soft read-out of every shifted crop
    (phase (0, 0) is the zoo itself, with every leaf; the other phases cut new blocks out of the same content)."""
    from test_gpu_dct_resync import device_crop, garbage
    from test_gpu_planar_resync import reference_scores
    marked = np.stack([ml.oracle_mark(f, WM, 20.0)[0] for f in zoo.frames])
    dev = cuda(marked)
    got = eng.sync_scores(dev, alpha=20, scores=garbage(2, 64)).cpu().numpy()
    ref = np.zeros((2, 64), np.int64)
    for py in range(8):
        for px in range(8):
            crop, (r, c) = device_crop(dev, py, px)
            ref[:, 8 * py + px] = eng.detect_soft(crop, r * c, alpha=20).abs().sum(dim=1).cpu().numpy()
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    for layout in LAYOUTS:
        planes = cuda(np.stack([orc.pack_yuv420(*orc.rgb_to_yuv420(f), layout) for f in marked]))
        gotp = eng.sync_scores_yuv420(planes, 128, 128, alpha=20, layout=layout, scores=garbage(2, 64)).cpu().numpy()
        refp = reference_scores(eng, "dct", planes, 128, 128, layout)
        assert np.array_equal(gotp, refp), (layout, np.argwhere(gotp != refp)[:5])
