"""GPU: C marked copies of 4:2:0 frames in one pass (ofmk_embed_copies_yuv420, ofmk_svd_embed_copies_yuv420) against the
single-copy planar calls, byte for byte: every copy equals the single-copy embed with that copy's watermark rows (blk 8's
fringe round trip included); the DwtDctSvd verify's counts and bits equal svd_embed_detect_yuv420's and svd_detect_yuv420's of
the copy; the chain through the RGB copies kernels gives the same planes; the fingerprint layer's one-pass route gives the
same copies and sidecars as the per-copy loop; the calls replay from a captured graph and are timed under their kinds.

Shapes: 8x8 is smaller than a 16x16 tile (blk 8 launches no tile kernel, every byte is fringe); 24x40 has blk 8's fringe on
both sides; 136x168 is 357 blocks = two workgroups, the last one partial, plus a fringe; 240x320 has none."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_WM = 5
SHAPES = [(8, 8, 1), (24, 40, 2), (136, 168, 3), (240, 320, 2)]
LAYOUTS = ["i420", "nv12"]
COPIES = [1, 2, 3, 16]
SCALES = [None, [5, 15, 20]]
_PLANES = {}


@pytest.fixture(scope="module")
def eng():
    import torch
    from offmark.engine import DctEngine
    torch.cuda.set_device(0)
    return DctEngine()


def planes_of(eng, shape, layout):
    """The shape's frames as planes (made once per shape and layout; no test writes into them)."""
    from offmark.synthetic import synthetic_frames
    key = (shape, layout)
    if key not in _PLANES:
        H, W, n = shape
        _PLANES[key] = eng.rgb_to_yuv420(synthetic_frames(n, H, W, seed=100 + H), layout)
    return _PLANES[key]


def wm_of(H, W, seed=7):
    import torch
    bits = np.random.default_rng(seed).integers(0, 2, (N_WM, H * W // 64), dtype=np.uint8)
    return torch.from_numpy(bits).cuda()


def rows_of(C, n, seed=11):
    """[C, n] device rows that vary per frame, out-of-range entries included (the kernels clamp them into [0, N_WM))."""
    import torch
    r = np.random.default_rng(seed).integers(-2, N_WM + 3, (C, n)).astype(np.int32)
    return torch.from_numpy(r).cuda()


def row_c(c, n):
    return np.full(n, min(c, N_WM - 1), np.int32)


@pytest.mark.parametrize("C", COPIES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_dct_copies_equal_single_copy_embed(eng, shape, layout, C):
    import torch
    from offmark.engine import DctEngine
    H, W, n = shape
    planes = planes_of(eng, shape, layout)
    before = planes.clone()
    wm, rows = wm_of(H, W), rows_of(C, n)
    out = eng.embed_copies_yuv420(planes, H, W, wm, rows, layout=layout)
    assert tuple(out.shape) == (C, n, H * W * 3 // 2)
    for c in range(C):
        assert torch.equal(out[c], eng.embed_yuv420(planes, H, W, wm, wm_row=rows[c], layout=layout)), c
    # no rows: copy c uses row c (clamped)
    out0 = eng.embed_copies_yuv420(planes, H, W, wm, None, copies=C, layout=layout)
    for c in range(C):
        assert torch.equal(out0[c], eng.embed_yuv420(planes, H, W, wm, wm_row=row_c(c, n), layout=layout)), c
    one = DctEngine(chunk_frames=1)                                 # chunks of one frame in a minimum workspace
    assert one.workspace(H, W, 1).numel() == one.lib.ofmk_workspace_bytes(1, H, W)
    assert torch.equal(one.embed_copies_yuv420(planes, H, W, wm, rows, layout=layout), out)
    assert torch.equal(planes, before)


@pytest.mark.parametrize("scales", SCALES)
@pytest.mark.parametrize("blk", [4, 8])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_svd_copies_equal_single_copy_calls(eng, shape, layout, blk, scales):
    import torch
    H, W, n = shape
    planes = planes_of(eng, shape, layout)
    before = planes.clone()
    wm = wm_of(H, W)
    kw = dict(scales=scales, blk=blk, layout=layout)
    tiles = int(eng.lib.ofmk_svd_count_tiles(H, W, blk))
    for C in COPIES:
        rows = rows_of(C, n, seed=13)
        out = eng.svd_embed_copies_yuv420(planes, H, W, wm, rows, **kw)
        assert tuple(out.shape) == (C, n, H * W * 3 // 2)
        for c in range(C):
            assert torch.equal(out[c], eng.svd_embed_yuv420(planes, H, W, wm, wm_row=rows[c], **kw)), (C, c)
        out_v, counts, bits = eng.svd_embed_copies_yuv420(planes, H, W, wm, rows, L=8, want_bits=True, **kw)
        assert torch.equal(out_v, out)
        assert tuple(counts.shape) == (C, n, 8) and tuple(bits.shape) == (C, n, eng.svd_bits_per_frame(H, W, blk))
        partial = None
        if tiles > 0:        # 8x8 with blk 8 has no workgroup, hence no partial rows: a [.., 0, L] buffer has no address to pass
            garbage = torch.full((C, n, tiles, 8), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            _, partial, _ = eng.svd_embed_copies_yuv420(planes, H, W, wm, rows, L=8, partial=True, counts=garbage, **kw)
            assert partial is garbage
        for c in range(C):
            _, rc, rb = eng.svd_embed_detect_yuv420(planes, H, W, wm, 8, wm_row=rows[c], want_bits=True, **kw)
            assert torch.equal(counts[c], rc) and torch.equal(bits[c], rb), (C, c)
            dc, db = eng.svd_detect_yuv420(out[c], H, W, 8, want_bits=True, **kw)
            assert torch.equal(counts[c], dc) and torch.equal(bits[c], db), (C, c)
            if partial is not None:
                assert torch.equal(eng.counts_from_partial(partial[c]), counts[c]), (C, c)
        out0 = eng.svd_embed_copies_yuv420(planes, H, W, wm, None, copies=C, **kw)
        for c in range(C):
            assert torch.equal(out0[c], eng.svd_embed_yuv420(planes, H, W, wm, wm_row=row_c(c, n), **kw)), (C, c)
    assert torch.equal(planes, before)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_copies_equal_the_chain_through_the_rgb_copies_kernels(eng, layout):
    """Follows from the single-copy contracts: planar call == rgb_to_yuv420(RGB call(yuv420_to_rgb(planes)))."""
    import torch
    shape = (136, 168, 3)
    H, W, n = shape
    planes = planes_of(eng, shape, layout)
    wm, rows = wm_of(H, W), rows_of(3, n, seed=15)
    rgb = eng.yuv420_to_rgb(planes, H, W, layout)
    got = eng.embed_copies_yuv420(planes, H, W, wm, rows, layout=layout)
    ref = eng.embed_copies(rgb, wm, rows)
    for c in range(3):
        assert torch.equal(got[c], eng.rgb_to_yuv420(ref[c], layout)), c
    for blk in (4, 8):
        for scales in SCALES:
            got = eng.svd_embed_copies_yuv420(planes, H, W, wm, rows, blk=blk, scales=scales, layout=layout)
            ref = eng.svd_embed_copies(rgb, wm, rows, blk=blk, scales=scales)
            for c in range(3):
                assert torch.equal(got[c], eng.rgb_to_yuv420(ref[c], layout)), (blk, scales, c)


def test_python_validation(eng):
    import torch
    shape = (24, 40, 2)
    H, W, n = shape
    planes = planes_of(eng, shape, "i420")
    wm, rows = wm_of(H, W), rows_of(3, n)
    for call in (eng.embed_copies_yuv420, eng.svd_embed_copies_yuv420):
        with pytest.raises(ValueError):
            call(planes, H, W, wm, rows_of(3, n + 1))                           # wrong wm_rows shape
        with pytest.raises(ValueError):
            call(planes, H, W, wm, rows[0])                                     # one-dimensional rows
        with pytest.raises(ValueError):
            call(planes, H, W, wm, np.full((2, n), N_WM, np.int32))             # host rows out of range
        with pytest.raises(ValueError):
            call(planes, H, W, wm, rows, out=torch.empty((2, n, H * W * 3 // 2), dtype=torch.uint8, device="cuda"))
        wide = torch.empty((3, n, H * W * 3), dtype=torch.uint8, device="cuda")[..., ::2]
        with pytest.raises(ValueError):
            call(planes, H, W, wm, rows, out=wide)                              # non-contiguous out
        with pytest.raises(ValueError):
            call(planes, H, W, wm, None, copies=17)
        with pytest.raises(ValueError):
            call(planes[:, :-8].contiguous(), H, W, wm, rows)                   # planes of the wrong length
        with pytest.raises(ValueError):
            call(planes, H, W, wm, rows, layout="yv12")


class _PerCopy:
    """The encoder with the one-pass methods hidden: mark_segment_copies_yuv420 falls back to its per-copy loop."""

    def __init__(self, enc):
        self._enc = enc

    def encode_planes_yuv420(self, *a, **k):
        return self._enc.encode_planes_yuv420(*a, **k)


@pytest.mark.parametrize("codec,blk", [("dct", 4), ("dwtdctsvd", 4), ("dwtdctsvd", 8)])
def test_mark_segment_copies_yuv420_one_pass_equals_per_copy(eng, codec, blk):
    import torch
    from offmark import fingerprint as fp
    from offmark.synthetic import synthetic_frames
    if codec == "dct":
        from offmark.embed.dct_encoder import DctEncoder
        from offmark.extract.dct_decoder import DctDecoder
        enc, dec, used = DctEncoder(), DctDecoder(), "encode_copies_planes_yuv420"
    else:
        from offmark.embed.dwt_dct_svd_encoder import DwtDctSvdEncoder
        from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder
        enc, dec, used = DwtDctSvdEncoder(blk=blk), DwtDctSvdDecoder(blk=blk), "encode_verify_copies_planes_yuv420"
    H, W, S, C, F = 240, 320, 4, 3, 6
    planes = eng.rgb_to_yuv420(synthetic_frames(S * F, H, W, seed=6000), "nv12")
    seg = np.repeat(np.arange(1, S + 1), F)
    calls = []
    real = getattr(enc, used)

    def spy(*a, **k):
        calls.append(used)
        return real(*a, **k)
    setattr(enc, used, spy)
    copies, side = fp.mark_segment_copies_yuv420(enc, dec, planes, H, W, seg, C, layout="nv12")
    assert calls == [used]
    ref_copies, ref_side = fp.mark_segment_copies_yuv420(_PerCopy(enc), dec, planes, H, W, seg, C, layout="nv12")
    assert calls == [used]
    assert side == ref_side and not side["failed_segments"]
    assert len(copies) == C and all(torch.equal(a, b) for a, b in zip(copies, ref_copies))
    assert all(tuple(m.shape) == (S * F, H * W * 3 // 2) for m in copies)
    base = copies[0].data_ptr()                                     # views of one [C, n, 1.5*H*W] tensor
    assert all(m.data_ptr() == base + c * S * F * (H * W * 3 // 2) for c, m in enumerate(copies))


def test_planar_copies_calls_replay_from_a_graph(eng):
    import torch
    shape, C = (136, 168, 3), 3
    H, W, n = shape
    planes = planes_of(eng, shape, "nv12")
    wm, rows = wm_of(H, W), rows_of(C, n, seed=14)
    kw = dict(layout="nv12")
    ref_dct = eng.embed_copies_yuv420(planes, H, W, wm, rows, **kw)
    ref_svd, ref_counts, _ = eng.svd_embed_copies_yuv420(planes, H, W, wm, rows, L=8, **kw)
    out_dct = torch.empty_like(ref_dct)
    out_svd = torch.empty_like(ref_svd)
    counts = torch.empty_like(ref_counts)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng.embed_copies_yuv420(planes, H, W, wm, rows, out=out_dct, **kw)       # warm-up on the capture stream
        eng.svd_embed_copies_yuv420(planes, H, W, wm, rows, out=out_svd, L=8, counts=counts, **kw)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            eng.embed_copies_yuv420(planes, H, W, wm, rows, out=out_dct, **kw)
            eng.svd_embed_copies_yuv420(planes, H, W, wm, rows, out=out_svd, L=8, counts=counts, **kw)
    torch.cuda.synchronize()
    out_dct.zero_()
    out_svd.zero_()
    counts.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_dct, ref_dct) and torch.equal(out_svd, ref_svd) and torch.equal(counts, ref_counts)
    del graph
    import gc
    gc.collect()
    torch.cuda.synchronize()


def test_launches_are_timed_under_their_kinds():
    import torch
    from offmark import _hip
    from offmark.engine import DctEngine
    shape, C = (24, 40, 2), 3
    H, W, n = shape
    tm = _hip.Timing(64)
    e = DctEngine(opts=tm.opts())
    planes = planes_of(e, shape, "i420")
    wm, rows = wm_of(H, W), rows_of(C, n)
    e.embed_copies_yuv420(planes, H, W, wm, rows)
    torch.cuda.synchronize()
    got = tm.collect()
    assert got["planar_analyze"]["launches"] == 1 and got["planar_mark"]["launches"] == 1       # kinds 5 and 6, one chunk
    assert got["planar_analyze"]["ms_total"] > 0 and got["planar_mark"]["ms_total"] > 0
    assert all(v["launches"] == 0 for k, v in got.items() if k not in ("planar_analyze", "planar_mark"))
    e.svd_embed_copies_yuv420(planes, H, W, wm, rows, blk=4)                    # one fused launch
    e.svd_embed_copies_yuv420(planes, H, W, wm, rows, blk=8, L=8)               # per copy: tiles + fringe
    torch.cuda.synchronize()
    got = tm.collect()
    tm.close()
    assert got["svd"]["launches"] == 1 + 2 * C and got["svd"]["ms_total"] > 0                  # kind 4
    assert all(v["launches"] == 0 for k, v in got.items() if k != "svd")
