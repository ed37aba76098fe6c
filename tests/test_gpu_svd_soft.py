"""GPU: the DwtDctSvd soft read-out (engine.svd_detect_soft / svd_detect_soft_yuv420) and the DCT codec's soft read-out on planes
(engine.detect_soft_yuv420).  Build extensions, not reference semantics; the reference's hard decision stays the default.

Reference: the NumPy statement of tests/_svd_soft.py -- the reference's decoder (float32 LAPACK) gives s0 per unit, the metric is
rint(-sin(2 pi s0 / scale) * 2^14) in float64.  Budget per position: the sum over its units of
    ceil(2 pi 2^14 / scale * 1e-3 * max(1, s0 / 100)) + 1
(1e-3 * max(1, s0 / 100): the project's bound on how far two float32 s0 of one block may differ, tests/test_gpu_svd.py:54;
2 pi 2^14 / scale: the metric's largest slope; +1: the rounding).  Everything that compares the device with itself (hard bits,
long payloads, planes, the plugin level) is exact.

OFFMARK_SOFT_PARITY_OUT=<file>: the parity test's worst deviation per unit next to its budget, one row per case
(profiles/svd_soft_parity.txt)."""
import functools
import os

import numpy as np
import pytest

import offmark_oracle as orc
import _svd_soft as ss
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
P8 = np.array([0, 1, 1, 0, 0, 1, 0, 1])
N = 3
SIZES = [(64, 96), (36, 52), (30, 44), (240, 320)]
GOLDEN_MARKED = {(64, 96, 4): "svd_syn_64x96", (36, 52, 4): "svd_syn_36x52", (30, 44, 4): "svd_syn_30x44",
                 (240, 320, 4): "svd_syn_240x320", (64, 96, 8): "svd_blk8_syn_64x96"}
_parity_rows = []


@pytest.fixture(scope="module")
def eng():
    import torch
    from offmark.engine import DctEngine
    torch.cuda.set_device(0)
    return DctEngine()


@pytest.fixture(scope="module", autouse=True)
def _parity_table():
    yield
    path = os.environ.get("OFFMARK_SOFT_PARITY_OUT")
    if path and _parity_rows:
        with open(path, "w") as f:
            f.write("# tests/test_gpu_svd_soft.py::test_parity_with_the_statement, L = units (the metric per unit), 3 frames per case:\n"
                    "# worst |device - statement| over the units, that unit's budget, the smallest budget of the case, and the worst\n"
                    "# deviation / budget ratio.  budget = ceil(2 pi 2^14 / scale * 1e-3 * max(1, s0 / 100)) + 1, scale 15.\n"
                    "# size      blk  units  worst_dev  its_budget  min_budget  worst_ratio  units_off_by_more_than_1\n")
            f.writelines(_parity_rows)


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()             # a copy: the shared references are read-only


def garbage(n, L):
    """The soft buffer a call gets holds anything: the library clears it."""
    import torch
    return torch.full((n, L), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")


def units_of(H, W, blk):
    return ((H // 4 * 2) // blk) * ((W // 4 * 2) // blk)


def oracle_marked(H, W, blk, seed):
    wm = orc.shuffle_generate(P8, (1, H * W // 64), 0)
    enc = orc.DwtDctSvdEncoderOracle(scales=(0, 15, 0), blk=blk)
    enc.read_wm(wm)
    return orc.mark_frame(orc.synthetic_frame(H, W, seed), enc)


@functools.lru_cache(maxsize=None)
def batch(H, W, blk):
    """3 marked frames of one size (the reference-run golden frame where there is one, oracle-marked synthetic frames) and the
    statement of each: (frames u8 [3, H, W, 3], s0 [3, units], m [3, units])."""
    frames = []
    if (H, W, blk) in GOLDEN_MARKED:
        frames.append(np.load(os.path.join(GOLDEN, GOLDEN_MARKED[(H, W, blk)] + ".npz"))["marked"])
    while len(frames) < N:
        frames.append(oracle_marked(H, W, blk, 3000 + 10 * blk + len(frames)))
    st = [ss.statement(f, blk=blk) for f in frames]
    out = np.stack(frames), np.stack([s["s0"] for s in st]), np.stack([s["m"] for s in st])
    for a in out:
        a.setflags(write=False)
    return out


def soft_call(eng, frames_dev, L, blk, **kw):
    return eng.svd_detect_soft(frames_dev, L, blk=blk, soft=garbage(frames_dev.shape[0], L), **kw)


# ---- 1. parity with the statement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blk", [4, 8])
@pytest.mark.parametrize("H,W", SIZES)
def test_parity_with_the_statement(eng, H, W, blk):
    frames, s0, m = batch(H, W, blk)
    units = units_of(H, W, blk)
    assert s0.shape == (N, units)
    dev = cuda(frames)
    for L in (8, 5, units):
        got = soft_call(eng, dev, L, blk).cpu().numpy()
        assert got.shape == (N, L) and got.dtype == np.int64
        for f in range(N):
            ref, bud = ss.regroup(m[f], L), ss.position_budget(s0[f], L)
            d = np.abs(got[f] - ref)
            print(f"{H}x{W} blk {blk} L {L} frame {f}: worst deviation {d.max()} (budget there {bud[d.argmax()]}, smallest budget {bud.min()})")
            assert (d <= bud).all(), (L, f, d.max(), bud[d.argmax()])
        if L == units:
            d = np.abs(got - m)
            bud = np.stack([ss.unit_budget(s0[f]) for f in range(N)])
            k = np.unravel_index(d.argmax(), d.shape)
            _parity_rows.append(f"{H:4d}x{W:<4d} {blk:4d} {units:6d} {d[k]:10d} {bud[k]:11d} {bud.min():11d} {(d / bud).max():12.3f} {(d > 1).sum():8d}\n")


# ---- 2. consistency with the hard read-out -----------------------------------------------------------------------------------
@pytest.mark.parametrize("blk", [4, 8])
@pytest.mark.parametrize("H,W", SIZES)
def test_sign_agrees_with_the_hard_bit_of_every_unit(eng, H, W, blk):
    frames, _, _ = batch(H, W, blk)
    units = units_of(H, W, blk)
    dev = cuda(frames)
    soft = soft_call(eng, dev, units, blk).cpu().numpy()
    _, bits = eng.svd_detect(dev, units, want_bits=True, blk=blk)
    bits = bits.cpu().numpy()[:, :units]
    assert (bits[soft > 0] == 1).all() and (bits[soft < 0] == 0).all()
    assert (soft != 0).mean() > 0.9                                   # ... and the statement above is not vacuous
    for scales in ((0, 0, 0), (10, 0, 20)):                            # channel 1 unmarked: zeros, as the hard read-out
        z = soft_call(eng, dev, 8, blk, scales=scales)
        assert z.shape == (N, 8) and not z.any()
    # there is no partial form: OFMK_F_PARTIAL_COUNTS is ignored
    from offmark import _hip
    from offmark.engine import DctEngine
    flagged = DctEngine(opts=_hip.Opts(_hip.F_PARTIAL_COUNTS, 0, None))
    assert np.array_equal(soft_call(flagged, dev, units, blk).cpu().numpy(), soft)


# ---- 3. long payloads: L > 2048 takes the global-atomic path, positions wrap ----------------------------------------------------
@pytest.mark.parametrize("blk", [4, 8])
def test_long_payload_equals_the_per_unit_result_regrouped(eng, blk):
    H, W, L = 384, 512, 2049
    units = units_of(H, W, blk)
    assert units == (3072 if blk == 4 else 768)
    dev = cuda(np.stack([orc.synthetic_frame(H, W, 4000 + i) for i in range(N)]))
    per_unit = soft_call(eng, dev, units, blk).cpu().numpy()
    got = soft_call(eng, dev, L, blk).cpu().numpy()
    assert np.abs(per_unit).max() <= 16384 and (per_unit != 0).mean() > 0.9
    for f in range(N):
        assert np.array_equal(got[f], ss.regroup(per_unit[f], L))


@pytest.mark.parametrize("planar", [False, True])
def test_frames_past_a_launch_chunk_get_their_own_rows(eng, planar):
    """More frames than one launch takes (65535): the second launch's frames and rows start where the first one's end."""
    import torch
    n, H, W, L, edge = 65537, 8, 8, 3, 65535
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    rgb = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    if planar:
        frames = eng.rgb_to_yuv420(rgb)
        call = lambda fr: eng.svd_detect_soft_yuv420(fr, H, W, L, soft=garbage(fr.shape[0], L))  # noqa: E731
    else:
        frames = rgb
        call = lambda fr: soft_call(eng, fr, L, 4)  # noqa: E731
    full = call(frames)
    assert torch.equal(full[edge - 3:], call(frames[edge - 3:].contiguous())) and torch.equal(full[:5], call(frames[:5].contiguous()))
    assert (full != 0).sum(dim=1).eq(1).float().mean() > 0.9           # one unit per frame: one non-zero position


# ---- 4. planes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["i420", "nv12"])
@pytest.mark.parametrize("blk", [4, 8])
@pytest.mark.parametrize("H,W", [(64, 96), (240, 320)])
def test_planes_equal_the_rgb_chain(eng, H, W, blk, layout):
    import torch
    frames, _, _ = batch(H, W, blk)
    planes = eng.rgb_to_yuv420(cuda(frames), layout=layout)
    rgb = eng.yuv420_to_rgb(planes, H, W, layout=layout)
    for L in (8, units_of(H, W, blk)):
        got = eng.svd_detect_soft_yuv420(planes, H, W, L, blk=blk, layout=layout, soft=garbage(N, L))
        ref = soft_call(eng, rgb, L, blk)
        assert got.dtype == torch.int64 and torch.equal(got, ref) and got.any()


@pytest.mark.parametrize("layout", ["i420", "nv12"])
@pytest.mark.parametrize("H,W", [(64, 96), (240, 320)])
def test_dct_soft_on_planes_equals_the_rgb_chain(eng, H, W, layout):
    import torch
    planes = eng.rgb_to_yuv420(cuda(np.stack([orc.synthetic_frame(H, W, 5000 + i) for i in range(N)])), layout=layout)
    rgb = eng.yuv420_to_rgb(planes, H, W, layout=layout)
    for L in (8, 5):
        got = eng.detect_soft_yuv420(planes, H, W, L, alpha=20, layout=layout, soft=garbage(N, L))
        ref = eng.detect_soft(rgb, L, alpha=20, soft=garbage(N, L))
        assert got.shape == (N, L) and torch.equal(got, ref) and got.any()


@pytest.mark.parametrize("H,W,layout", [(64, 96, None), (36, 52, None), (64, 96, "i420"), (64, 96, "nv12"), (240, 320, "i420"),
                                        (240, 320, "nv12")])
def test_dct_soft_does_not_depend_on_the_workspace_chunk(eng, H, W, layout):
    """3 frames in workspace chunks of 1 and of 2 (2 + 1) give the sums of the default engine's single chunk; layout None: RGB
    frames (36x52: fringe and unaligned rows), else planes."""
    import torch
    from offmark.engine import DctEngine
    rgb = cuda(np.stack([orc.synthetic_frame(H, W, 5100 + i) for i in range(N)]))
    if layout is None:
        call = lambda e, L: e.detect_soft(rgb, L, alpha=20, soft=garbage(N, L))  # noqa: E731
    else:
        planes = eng.rgb_to_yuv420(rgb, layout=layout)
        call = lambda e, L: e.detect_soft_yuv420(planes, H, W, L, alpha=20, layout=layout, soft=garbage(N, L))  # noqa: E731
    for L in (8, 5):
        ref = call(eng, L)
        assert ref.shape == (N, L) and ref.dtype == torch.int64 and ref.any()
        for chunk in (1, 2):
            assert torch.equal(call(DctEngine(chunk_frames=chunk), L), ref), (L, chunk)


# ---- 5. usefulness: the noise recipe of tests/test_svd_soft_statement.py through the device ----------------------------------
def test_soft_sums_recover_segments_the_hard_vote_loses(eng):
    from offmark.degenerator.de_shuffler import DeShuffler
    from offmark.dist.vote import soft_vote, vote_segments
    r = ss.noise_recipe()
    S, F, L = ss.SEGMENTS, ss.FRAMES, ss.L8
    dev = cuda(r["noisy"].reshape(S * F, ss.H, ss.W, 3))
    seg = np.repeat(np.arange(S), F)
    soft = soft_call(eng, dev, L, 4).cpu().numpy()
    d = np.abs(soft - r["soft"].reshape(S * F, L))
    print(f"worst deviation from the statement {d.max()} (smallest position budget {r['budget'].min()})")
    assert (d <= r["budget"].reshape(S * F, L)).all()
    deg = DeShuffler(key=0).set_shape((L,))
    by_soft = soft_vote(soft, deg.payload_idx, seg)
    n_soft = sum(int(np.array_equal(by_soft[s], r["payloads"][s])) for s in range(S))
    counts, _ = eng.svd_detect(dev, L)
    patterns = deg.degenerate_counts(counts.cpu().numpy(), ss.H * ss.W // 64)
    by_hard = vote_segments(patterns, seg)
    n_hard = sum(int(np.array_equal(by_hard[s][0], r["payloads"][s])) for s in range(S))
    print(f"segments recovered: soft sums {n_soft}/16, hard decision with mode vote {n_hard}/16")
    assert n_soft == 16 and n_hard < n_soft


# ---- 6. plugin level ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pix_fmt", ["rgb24", "yuv420p"])
def test_extractor_brings_the_soft_sums_back(eng, pix_fmt):
    from offmark.degenerator.de_shuffler import DeShuffler
    from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder
    from offmark.generator.shuffler import Shuffler
    from offmark.video.extractor import Extractor
    from offmark.video.frame_reader import ArrayFrameReader
    H, W, n, L = 240, 320, 11, 8
    wm = Shuffler(key=0).generate_wm(P8, (1, H * W // 64))
    src = cuda(np.stack([orc.synthetic_frame(H, W, 6000 + i) for i in range(n)]))
    if pix_fmt == "rgb24":
        marked = eng.svd_embed(src, wm)
        direct = eng.svd_detect_soft(marked, L).cpu().numpy()
        clip = marked.cpu().numpy()
    else:
        marked = eng.svd_embed_yuv420(eng.rgb_to_yuv420(src), H, W, wm)
        direct = eng.svd_detect_soft_yuv420(marked, H, W, L).cpu().numpy()
        clip = marked.cpu().numpy().reshape(n, H * 3 // 2, W)
    deg = lambda: DeShuffler(key=0).set_shape((L,))  # noqa: E731
    ex = Extractor(ArrayFrameReader(clip, pix_fmt=pix_fmt), DwtDctSvdDecoder(), deg(), batch_frames=4, soft=True)
    ex.start()
    plain = Extractor(ArrayFrameReader(clip, pix_fmt=pix_fmt), DwtDctSvdDecoder(), deg(), batch_frames=4)
    plain.start()
    assert ex.soft_sums.shape == (n, L) and ex.soft_sums.dtype == np.int64 and np.array_equal(ex.soft_sums, direct)
    assert len(ex.patterns) == n and all(np.array_equal(a, b) for a, b in zip(ex.patterns, plain.patterns))
    assert np.array_equal(ex.soft_payload(), P8)
    assert plain.soft_sums is None
    with pytest.raises(ValueError):
        plain.soft_payload()
