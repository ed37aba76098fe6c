"""GPU: C marked copies in one pass (ofmk_embed_copies_rgb8, ofmk_svd_embed_copies_rgb8) against the single-copy calls, byte for
byte: every copy equals the single-copy embed with that copy's watermark rows, fringe pixels included; the DwtDctSvd verify's
counts and bits equal svd_embed_detect's and svd_detect's of the copy; the fingerprint layer's one-pass route gives the same
copies and sidecars as the per-copy loop; and the calls replay from a captured graph."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_WM = 5


@pytest.fixture(scope="module")
def eng():
    import torch
    from offmark.engine import DctEngine
    torch.cuda.set_device(0)
    return DctEngine()


def frames_of(n, H, W, seed):
    from offmark.synthetic import synthetic_frames
    return synthetic_frames(n, H, W, seed=seed)


def wm_of(H, W, seed=7):
    import torch
    bits = np.random.default_rng(seed).integers(0, 2, (N_WM, H * W // 64), dtype=np.uint8)
    return torch.from_numpy(bits).cuda()


def rows_of(C, n, seed=11):
    """[C, n] device rows that vary per frame, out-of-range entries included (the kernels clamp them into [0, N_WM))."""
    import torch
    r = np.random.default_rng(seed).integers(-2, N_WM + 3, (C, n)).astype(np.int32)
    return torch.from_numpy(r).cuda()


DCT_SHAPES = [(240, 320, 3), (1080, 1920, 2), (250, 330, 3)]


@pytest.mark.parametrize("C", [1, 2, 3, 16])
@pytest.mark.parametrize("shape", DCT_SHAPES)
def test_dct_copies_equal_single_copy_embed(eng, shape, C):
    import torch
    H, W, n = shape
    frames = frames_of(n, H, W, 100 + H)
    before = frames.clone()
    wm, rows = wm_of(H, W), rows_of(C, n)
    out = eng.embed_copies(frames, wm, rows)
    assert tuple(out.shape) == (C, n, H, W, 3)
    for c in range(C):
        assert torch.equal(out[c], eng.embed(frames, wm, wm_row=rows[c])), c
    # no rows: copy c uses row c (clamped)
    out0 = eng.embed_copies(frames, wm, None, copies=C)
    for c in range(C):
        assert torch.equal(out0[c], eng.embed(frames, wm, wm_row=np.full(n, min(c, N_WM - 1), np.int32))), c
    assert torch.equal(frames, before)


@pytest.mark.parametrize("shape", DCT_SHAPES)
def test_dct_copies_do_not_depend_on_chunks_workspace_or_tile_order(eng, shape):
    import torch
    from offmark.engine import DctEngine
    H, W, n = shape
    frames = frames_of(n, H, W, 200 + W)
    wm, rows = wm_of(H, W), rows_of(3, n, seed=12)
    ref = eng.embed_copies(frames, wm, rows)
    one = DctEngine(chunk_frames=1)                                 # chunks of one frame in a minimum workspace
    assert one.workspace(H, W, 1).numel() == one.lib.ofmk_workspace_bytes(1, H, W)
    assert torch.equal(one.embed_copies(frames, wm, rows), ref)
    for order in ("linear", "xcd"):
        assert torch.equal(DctEngine(tile_order=order).embed_copies(frames, wm, rows), ref), order


SVD_SHAPES = [(240, 320, 3), (250, 330, 2)]
SCALES = [None, [5, 15, 20]]


@pytest.mark.parametrize("C", [1, 2, 3, 16])
@pytest.mark.parametrize("scales", SCALES)
@pytest.mark.parametrize("blk", [4, 8])
@pytest.mark.parametrize("shape", SVD_SHAPES)
def test_svd_copies_equal_single_copy_calls(eng, shape, blk, scales, C):
    import torch
    H, W, n = shape
    frames = frames_of(n, H, W, 300 + H)
    before = frames.clone()
    wm, rows = wm_of(H, W), rows_of(C, n, seed=13)
    kw = dict(scales=scales, blk=blk)
    out = eng.svd_embed_copies(frames, wm, rows, **kw)
    assert tuple(out.shape) == (C, n, H, W, 3)
    for c in range(C):
        assert torch.equal(out[c], eng.svd_embed(frames, wm, wm_row=rows[c], **kw)), c
    out_v, counts, bits = eng.svd_embed_copies(frames, wm, rows, L=8, want_bits=True, **kw)
    assert torch.equal(out_v, out)
    assert tuple(counts.shape) == (C, n, 8) and tuple(bits.shape) == (C, n, eng.svd_bits_per_frame(H, W, blk))
    _, partial, _ = eng.svd_embed_copies(frames, wm, rows, L=8, partial=True, **kw)
    for c in range(C):
        _, rc, rb = eng.svd_embed_detect(frames, wm, 8, wm_row=rows[c], want_bits=True, **kw)
        assert torch.equal(counts[c], rc) and torch.equal(bits[c], rb), c
        dc, db = eng.svd_detect(out[c].contiguous(), 8, want_bits=True, **kw)
        assert torch.equal(counts[c], dc) and torch.equal(bits[c], db), c
        assert torch.equal(eng.counts_from_partial(partial[c]), counts[c]), c
    out0 = eng.svd_embed_copies(frames, wm, None, copies=C, **kw)
    for c in range(C):
        assert torch.equal(out0[c], eng.svd_embed(frames, wm, wm_row=np.full(n, min(c, N_WM - 1), np.int32), **kw)), c
    assert torch.equal(frames, before)


def test_python_validation(eng):
    import torch
    H, W, n = 64, 96, 2
    frames = frames_of(n, H, W, 5)
    wm, rows = wm_of(H, W), rows_of(3, n)
    for call in (eng.embed_copies, eng.svd_embed_copies):
        with pytest.raises(ValueError):
            call(frames, wm, rows_of(3, n + 1))                                 # wrong wm_rows shape
        with pytest.raises(ValueError):
            call(frames, wm, rows[0])                                           # one-dimensional rows
        with pytest.raises(ValueError):
            call(frames, wm, np.full((2, n), N_WM, np.int32))                   # host rows out of range
        with pytest.raises(ValueError):
            call(frames, wm, rows, out=torch.empty((2, n, H, W, 3), dtype=torch.uint8, device="cuda"))
        wide = torch.empty((3, n, H, W, 6), dtype=torch.uint8, device="cuda")[..., :3]
        with pytest.raises(ValueError):
            call(frames, wm, rows, out=wide)                                    # non-contiguous out
        with pytest.raises(ValueError):
            call(frames, wm, None, copies=17)


class _PerCopy:
    """The encoder with the one-pass methods hidden: mark_segment_copies falls back to its per-copy loop."""

    def __init__(self, enc):
        self._enc = enc

    def encode_frames_u8(self, *a, **k):
        return self._enc.encode_frames_u8(*a, **k)


@pytest.mark.parametrize("codec,blk", [("dct", 4), ("dwtdctsvd", 4), ("dwtdctsvd", 8)])
def test_mark_segment_copies_one_pass_equals_per_copy(codec, blk):
    import torch
    from offmark import fingerprint as fp
    if codec == "dct":
        from offmark.embed.dct_encoder import DctEncoder
        from offmark.extract.dct_decoder import DctDecoder
        enc, dec, used = DctEncoder(), DctDecoder(), "encode_copies_u8"
    else:
        from offmark.embed.dwt_dct_svd_encoder import DwtDctSvdEncoder
        from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder
        enc, dec, used = DwtDctSvdEncoder(blk=blk), DwtDctSvdDecoder(blk=blk), "encode_verify_copies_u8"
    H, W, S, C, F = 240, 320, 4, 3, 6
    frames = frames_of(S * F, H, W, 6000)
    seg = np.repeat(np.arange(1, S + 1), F)
    calls = []
    real = getattr(enc, used)

    def spy(*a, **k):
        calls.append(used)
        return real(*a, **k)
    setattr(enc, used, spy)
    copies, side = fp.mark_segment_copies(enc, dec, frames, seg, C)
    assert calls == [used]
    ref_copies, ref_side = fp.mark_segment_copies(_PerCopy(enc), dec, frames, seg, C)
    assert calls == [used]
    assert side == ref_side and not side["failed_segments"]
    assert len(copies) == C and all(torch.equal(a, b) for a, b in zip(copies, ref_copies))


def test_copies_calls_replay_from_a_graph(eng):
    import torch
    H, W, n, C = 240, 320, 3, 3
    frames = frames_of(n, H, W, 900)
    wm, rows = wm_of(H, W), rows_of(C, n, seed=14)
    ref_dct = eng.embed_copies(frames, wm, rows)
    ref_svd, ref_counts, _ = eng.svd_embed_copies(frames, wm, rows, L=8)
    out_dct = torch.empty_like(ref_dct)
    out_svd = torch.empty_like(ref_svd)
    counts = torch.empty_like(ref_counts)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng.embed_copies(frames, wm, rows, out=out_dct)                          # warm-up on the capture stream
        eng.svd_embed_copies(frames, wm, rows, out=out_svd, L=8, counts=counts)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            eng.embed_copies(frames, wm, rows, out=out_dct)
            eng.svd_embed_copies(frames, wm, rows, out=out_svd, L=8, counts=counts)
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
