"""GPU: the DwtDctSvd codec on planar 8-bit YUV 4:2:0 (I420 / NV12 in, the same out): ofmk_svd_*_yuv420, the engine's
svd_*_yuv420, DwtDctSvdEncoder.encode_planes_yuv420 / DwtDctSvdDecoder.decode_planes_yuv420 and the Embedder / Extractor
route through them.

What is pinned:
  * fused planar calls against the chain convert -> RGB DwtDctSvd call -> convert ..... bit-exact (pixels, counts, bits,
    partial counts, payloads, in place), blk 4 and 8, the blk 8 fringe (the chain's planes -> RGB -> planes round trip)
  * the planar path against the oracle pipeline (oracle conversion around the oracle's mark_frame) ..... tests/test_gpu_svd.py's
    budgets: <= 1 LSB on <= 2e-5 of the samples over determined tiles (counted over the frame's RGB samples, 3 per pixel),
    raw bits <= 1e-4 of the blocks, payloads after DeShuffler bit-exact
  * the plugin methods and the pipeline take the fused path (no conversion call) and give the chain's bytes and payloads
  * timing: every launch counts under "svd" (blk 8 with a fringe: one more launch per embed)
"""
import numpy as np
import pytest

import offmark_oracle as orc

pytestmark = pytest.mark.gpu
P8 = np.array([0, 1, 1, 0, 0, 1, 0, 1])
L = 8
LAYOUTS = ["i420", "nv12"]
FMT = {"i420": "yuv420p", "nv12": "nv12"}


@pytest.fixture(scope="module")
def eng():
    import torch
    from offmark.engine import DctEngine
    torch.cuda.set_device(0)
    return DctEngine()


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def budget(n, frac, floor=1):
    return max(floor, int(np.floor(n * frac)))


def planes_of(rgb_frames, layout):
    return np.stack([orc.pack_yuv420(*orc.rgb_to_yuv420(f), layout) for f in rgb_frames])


def rgb_of(planes, H, W, layout):
    return orc.yuv420_to_rgb(*orc.unpack_yuv420(planes, H, W, layout))


def frames_rgb(n, H, W, seed=1001):
    if H >= 16 and W >= 16:
        return np.stack([orc.synthetic_frame(H, W, seed + i) for i in range(n)])
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def wm_table(N):
    return np.stack([orc.shuffle_generate(np.roll(P8, i), (1, N), 0)[0] for i in range(3)]).astype(np.uint8)


SHAPES = [(240, 320, 9), (1080, 1920, 4), (8, 8, 1), (16, 264, 3), (24, 40, 2)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("scales", [(0, 15, 0), (8, 22, 8)], ids=["default", "multi"])
@pytest.mark.parametrize("blk", [4, 8])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_fused_equals_the_chain_bit_for_bit(eng, layout, blk, scales, shape):
    import torch
    H, W, n = shape
    planes = cuda(planes_of(frames_rgb(n, H, W), layout))
    wm = cuda(wm_table(H * W // 64))
    rows = np.arange(n) % 3
    kw = dict(scales=scales, blk=blk)
    # the chain
    rgb_out = eng.svd_embed(eng.yuv420_to_rgb(planes, H, W, layout), wm, wm_row=rows, **kw)
    chain = eng.rgb_to_yuv420(rgb_out, layout)
    c_counts, c_bits = eng.svd_detect(eng.yuv420_to_rgb(chain, H, W, layout), L, want_bits=True, **kw)
    # fused
    out = eng.svd_embed_yuv420(planes, H, W, wm, wm_row=rows, layout=layout, **kw)
    assert torch.equal(out, chain)
    counts, bits = eng.svd_detect_yuv420(out, H, W, L, want_bits=True, layout=layout, **kw)
    assert torch.equal(counts, c_counts) and torch.equal(bits, c_bits)
    assert bits.shape == (n, H * W // (4 * blk * blk))
    out2, counts2, bits2 = eng.svd_embed_detect_yuv420(planes, H, W, wm, L, wm_row=rows, want_bits=True, layout=layout, **kw)
    assert torch.equal(out2, chain) and torch.equal(counts2, c_counts) and torch.equal(bits2, c_bits)
    # partial counts (a frame with no tile has no partial rows: nothing to check there)
    tiles = eng.lib.ofmk_svd_count_tiles(H, W, blk)
    perm = torch.as_tensor(orc.payload_permutation(L, 0), dtype=torch.int32).cuda()
    n_bits = eng.svd_bits_per_frame(H, W, blk)
    if tiles > 0:
        p_det, _ = eng.svd_detect_yuv420(out, H, W, L, partial=True, layout=layout, **kw)
        _, p_ed, _ = eng.svd_embed_detect_yuv420(planes, H, W, wm, L, wm_row=rows, partial=True, layout=layout, **kw)
        assert p_det.shape == (n, tiles, L)
        assert torch.equal(p_det.sum(1, dtype=torch.int32), c_counts) and torch.equal(p_ed, p_det)
        if n_bits:
            assert torch.equal(eng.payloads(p_det, n_bits, perm), eng.payloads(c_counts, n_bits, perm))
    # in place
    buf = planes.clone()
    assert eng.svd_embed_yuv420(buf, H, W, wm, wm_row=rows, out=buf, layout=layout, **kw) is buf
    assert torch.equal(buf, chain)
    buf = planes.clone()
    _, counts3, bits3 = eng.svd_embed_detect_yuv420(buf, H, W, wm, L, wm_row=rows, out=buf, want_bits=True, layout=layout, **kw)
    assert torch.equal(buf, chain) and torch.equal(counts3, c_counts) and torch.equal(bits3, c_bits)
    # blk 8: the uncovered fringe is the input's 4:2:0 round trip, not the input bytes
    if blk == 8:
        rt = eng.rgb_to_yuv420(eng.yuv420_to_rgb(planes, H, W, layout), layout).cpu().numpy()
        Hc, Wc = (H // 16) * 16, (W // 16) * 16
        for f in range(n):
            got_y = orc.unpack_yuv420(out[f].cpu().numpy(), H, W, layout)[0]
            rt_y = orc.unpack_yuv420(rt[f], H, W, layout)[0]
            assert np.array_equal(got_y[Hc:], rt_y[Hc:]) and np.array_equal(got_y[:, Wc:], rt_y[:, Wc:])


def _oracle_case(frame, layout, blk):
    from test_gpu_svd import determined_pixels
    H, W, _ = frame.shape
    planes = orc.pack_yuv420(*orc.rgb_to_yuv420(frame), layout)
    rgb_in = rgb_of(planes, H, W, layout)
    wm = orc.shuffle_generate(P8, (1, H * W // 64), 0)
    enc = orc.DwtDctSvdEncoderOracle(blk=blk)
    enc.read_wm(wm)
    ref_planes = orc.pack_yuv420(*orc.rgb_to_yuv420(orc.mark_frame(rgb_in, enc)), layout)
    mask, ok = determined_pixels(rgb_in, wm, blk=blk)
    return planes, wm, ref_planes, mask, ok


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("which", ["frame63", "synthetic", "synthetic_blk8"])
def test_planar_path_against_the_oracle_pipeline(eng, layout, which):
    from conftest import natural_frame
    from offmark.degenerator.de_shuffler import DeShuffler
    frame = natural_frame() if which == "frame63" else orc.synthetic_frame(240, 320, 2000)
    blk = 8 if which.endswith("blk8") else 4
    H, W, _ = frame.shape
    planes, wm, ref_planes, mask, ok = _oracle_case(frame, layout, blk)
    n_bits = H * W // (4 * blk * blk)
    out, counts, _ = eng.svd_embed_detect_yuv420(cuda(planes[None]), H, W, wm, L, want_bits=True, blk=blk, layout=layout)
    got = out[0].cpu().numpy()
    gy, gu, gv = orc.unpack_yuv420(got, H, W, layout)
    ry, ru, rv = orc.unpack_yuv420(ref_planes, H, W, layout)
    cmask = mask[::2, ::2]                                     # tiles are aligned to the 2x2 chroma grid
    d = np.concatenate([np.abs(gy.astype(int) - ry)[mask], np.abs(gu.astype(int) - ru)[cmask], np.abs(gv.astype(int) - rv)[cmask]])
    assert d.max() <= 1, d.max()
    assert (d > 0).sum() <= budget(3 * int(mask.sum()), 2e-5), (d > 0).sum()
    # raw bits: the fused read-out of the oracle's planes against the oracle's decoder on the same planes
    ref_bits = orc.check_frame(rgb_of(ref_planes, H, W, layout), orc.DwtDctSvdDecoderOracle(blk=blk)).reshape(-1)
    _, b2 = eng.svd_detect_yuv420(cuda(ref_planes[None]), H, W, L, want_bits=True, blk=blk, layout=layout)
    assert (b2[0].cpu().numpy() != ref_bits).sum() <= budget(ok.size, 1e-4)
    # payloads: the verify (a reader of the written planes, after their own 4:2:0 round trip) and the oracle's read-out of them
    deg = DeShuffler(key=0).set_shape(P8.shape)
    assert np.array_equal(deg.degenerate_counts(counts[0].cpu().numpy(), n_bits), P8)
    ours_read = orc.check_frame(rgb_of(got, H, W, layout), orc.DwtDctSvdDecoderOracle(blk=blk))
    assert np.array_equal(orc.deshuffle(ours_read, L, 0), P8)


@pytest.mark.parametrize("blk", [4, 8])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_plugins_and_pipeline_take_the_fused_path(eng, layout, blk, monkeypatch):
    import torch
    from offmark.degenerator.de_shuffler import DeShuffler
    from offmark.embed.dwt_dct_svd_encoder import DwtDctSvdEncoder
    from offmark.engine import DctEngine
    from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder
    from offmark.generator.shuffler import Shuffler
    from offmark.video.embedder import Embedder
    from offmark.video.extractor import Extractor
    from offmark.video.frame_reader import ArrayFrameReader
    from offmark.video.frame_writer import ArrayFrameWriter
    H, W, n, B = 48, 80, 7, 3                              # blk 8: a fringe row and column of 8x8 blocks
    enc, dec = DwtDctSvdEncoder(blk=blk), DwtDctSvdDecoder(blk=blk)
    enc.read_wm(Shuffler(key=0).generate_wm(P8, enc.wm_capacity((H, W, 3))))
    planes = cuda(planes_of(frames_rgb(n, H, W, 77), layout))
    wm = enc._device_wm(H * W // 64)
    n_bits = dec.bits_per_frame(H, W)
    # the chain, before the conversions are taken away
    chain = eng.rgb_to_yuv420(eng.svd_embed(eng.yuv420_to_rgb(planes, H, W, layout), wm, blk=blk), layout)
    c_counts, c_bits = eng.svd_detect(eng.yuv420_to_rgb(chain, H, W, layout), L, want_bits=True, blk=blk)
    want_payloads = DeShuffler(key=0).set_shape(P8.shape).degenerate_counts(c_counts.cpu().numpy(), n_bits)

    def no_conversion(*a, **k):
        raise AssertionError("the planar DwtDctSvd path converted to RGB")
    monkeypatch.setattr(DctEngine, "yuv420_to_rgb", no_conversion)
    monkeypatch.setattr(DctEngine, "rgb_to_yuv420", no_conversion)
    out = enc.encode_planes_yuv420(planes, H, W, layout=layout)
    assert torch.equal(out, chain)
    assert torch.equal(out, eng.svd_embed_yuv420(planes, H, W, wm, blk=blk, layout=layout))
    counts, bits = dec.decode_planes_yuv420(out, H, W, L, want_bits=True, layout=layout)
    assert torch.equal(counts, c_counts) and torch.equal(bits, c_bits)
    e_counts, e_bits = eng.svd_detect_yuv420(out, H, W, L, want_bits=True, blk=blk, layout=layout)
    assert torch.equal(counts, e_counts) and torch.equal(bits, e_bits)
    fmt = FMT[layout]
    src = planes.cpu().numpy().reshape(n, H * 3 // 2, W)
    wr = ArrayFrameWriter(pix_fmt=fmt)
    Embedder(ArrayFrameReader(src, pix_fmt=fmt), enc, wr, batch_frames=B).start()
    got = np.stack(wr.frames)
    assert np.array_equal(got.reshape(n, -1), chain.cpu().numpy())
    ex = Extractor(ArrayFrameReader(got, pix_fmt=fmt), dec, DeShuffler(key=0).set_shape(P8.shape), batch_frames=B)
    ex.start()
    assert np.array_equal(np.stack(ex.patterns), want_payloads)
    if n_bits >= 64:
        assert all(np.array_equal(p, P8) for p in ex.patterns)


@pytest.mark.parametrize("blk,shape,svd_launches", [(4, (240, 320), 3), (8, (240, 320), 3), (8, (24, 40), 5)])
def test_launches_are_timed_as_svd(blk, shape, svd_launches):
    import torch
    from offmark import _hip
    from offmark.engine import DctEngine
    H, W = shape
    tm = _hip.Timing(64)
    e = DctEngine(opts=tm.opts())
    planes = cuda(planes_of(frames_rgb(2, H, W), "nv12"))
    wm = wm_table(H * W // 64)[:1]
    out = e.svd_embed_yuv420(planes, H, W, wm, blk=blk, layout="nv12")
    e.svd_detect_yuv420(out, H, W, L, blk=blk, layout="nv12")
    e.svd_embed_detect_yuv420(planes, H, W, wm, L, blk=blk, layout="nv12")
    torch.cuda.synchronize()
    got = tm.collect()
    tm.close()
    assert got["svd"]["launches"] == svd_launches and got["svd"]["ms_total"] > 0
    assert all(v["launches"] == 0 for k, v in got.items() if k != "svd")
