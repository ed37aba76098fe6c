"""GPU: the one-pass copies calls with the soft read-out of every copy (ofmk_embed_detect_copies_soft_rgb8,
ofmk_svd_embed_copies_soft_rgb8, ofmk_svd_embed_copies_soft_yuv420; engine ``soft=``) against calls that exist without them, integer for
integer: out / counts / bits equal the copies call without ``soft``, soft[c] equals the stand-alone soft read-out of the written copy;
nothing depends on the payload length's path, on what the destinations held, on chunking, tile order or the separate route; the
launches are the counterparts'; the calls replay from a graph; and the fingerprint layer turns the sums into per-(segment, copy)
margins that equal copy_margins of the per-copy soft read-outs.

Shapes are the smallest that reach each path.  RGB: 16x24 is 6 blocks (one ragged tile), n = 3 against chunks of 2; 250x330 has
unaligned rows, a fringe and a ragged last tile.  Planes: 8x8 is smaller than a blk-8 tile, 24x40 has a blk-8 fringe, 136x168 is
two workgroups, the last one partial.  L = 5 is no power of two, L = 4096 is above the LDS histograms (small shapes only)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_WM = 5
RGB_SHAPES = [(16, 24, 3), (64, 96, 2), (250, 330, 3)]
PLANAR_SHAPES = [(8, 8, 1), (24, 40, 2), (136, 168, 3)]
LAYOUTS = ["i420", "nv12"]
COPIES = [1, 3, 16]
SCALES = [None, [5, 15, 20]]
_PLANES = {}


@pytest.fixture(scope="module")
def eng():
    import torch
    from offmark.engine import DctEngine
    torch.cuda.set_device(0)
    return DctEngine()


def lengths(shape, small):
    return (8, 5, 4096) if shape in small else (8, 5)


def frames_of(n, H, W, seed):
    from offmark.synthetic import synthetic_frames
    return synthetic_frames(n, H, W, seed=seed)


def planes_of(eng, shape, layout):
    key = (shape, layout)
    if key not in _PLANES:
        H, W, n = shape
        _PLANES[key] = eng.rgb_to_yuv420(frames_of(n, H, W, 100 + H), layout)
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


def same(got, ref):
    import torch
    return len(got) == len(ref) and all((a is None and b is None) or torch.equal(a, b) for a, b in zip(got, ref))


def check(got, ref, soft_of, C):
    """got = (out, counts, bits, soft) of a call with soft; ref = the call without; soft_of(copy) = the stand-alone soft read-out."""
    import torch
    assert len(got) == 4 and same(got[:3], ref)
    soft = got[3]
    assert soft.dtype == torch.int64 and soft.shape[0] == C
    for c in range(C):
        assert torch.equal(soft[c], soft_of(got[0][c].contiguous())), c


# ---- the three calls against the calls without soft and the stand-alone soft read-outs ----------------------------------------
@pytest.mark.parametrize("C", COPIES)
@pytest.mark.parametrize("shape", RGB_SHAPES)
def test_dct_call(eng, shape, C):
    import torch
    H, W, n = shape
    frames = frames_of(n, H, W, 100 + H + C)
    before = frames.clone()
    wm, rows = wm_of(H, W), rows_of(C, n)
    for L in lengths(shape, RGB_SHAPES[:2]):
        ref = eng.embed_detect_copies(frames, wm, rows, L, want_bits=True)
        got = eng.embed_detect_copies(frames, wm, rows, L, want_bits=True, soft=True)
        assert tuple(got[3].shape) == (C, n, L)
        check(got, ref, lambda copy: eng.detect_soft(copy, L), C)
    ref = eng.embed_detect_copies(frames, wm, None, 8, want_bits=True, copies=C)               # no rows: copy c uses row c (clamped)
    check(eng.embed_detect_copies(frames, wm, None, 8, want_bits=True, copies=C, soft=True), ref, lambda copy: eng.detect_soft(copy, 8), C)
    if C == 1:                                                      # the single-copy embed plus the soft detect of its output
        one = eng.embed(frames, wm, wm_row=torch.zeros(n, dtype=torch.int32, device="cuda"))
        got = eng.embed_detect_copies(frames, wm, None, 8, copies=1, soft=True)
        assert torch.equal(got[0][0], one) and torch.equal(got[3][0], eng.detect_soft(one, 8))
    assert torch.equal(frames, before)


def svd_case(call, soft_of, count_tiles, C, n, Ls, **kw):
    import torch
    rows = rows_of(C, n, seed=13)
    for L in Ls:
        ref = call(rows, L=L, want_bits=True, **kw)
        got = call(rows, L=L, want_bits=True, soft=True, **kw)
        assert tuple(got[3].shape) == (C, n, L)
        check(got, ref, lambda copy: soft_of(copy, L), C)
        if count_tiles > 0 and L <= 2048:                           # the partial-counts form while soft is also requested
            garbage = torch.full((C, n, count_tiles, L), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            part = call(rows, L=L, partial=True, counts=garbage, soft=True, **kw)
            assert part[1] is garbage and torch.equal(part[0], ref[0]) and torch.equal(part[3], got[3])
            assert torch.equal(call(rows, L=L, partial=True, **kw)[1], garbage)
    ref = call(None, L=8, want_bits=True, copies=C, **kw)
    check(call(None, L=8, want_bits=True, copies=C, soft=True, **kw), ref, lambda copy: soft_of(copy, 8), C)


@pytest.mark.parametrize("scales", SCALES)
@pytest.mark.parametrize("blk", [4, 8])
@pytest.mark.parametrize("shape", RGB_SHAPES)
def test_svd_rgb_call(eng, shape, blk, scales):
    import torch
    H, W, n = shape
    frames = frames_of(n, H, W, 200 + H)
    before = frames.clone()
    wm = wm_of(H, W)
    kw = dict(scales=scales, blk=blk)
    tiles = int(eng.lib.ofmk_svd_count_tiles(H, W, blk))
    for C in COPIES:
        svd_case(lambda rows, **k: eng.svd_embed_copies(frames, wm, rows, **k), lambda copy, L: eng.svd_detect_soft(copy, L, **kw),
                 tiles, C, n, lengths(shape, RGB_SHAPES[:2]), **kw)
    one = eng.svd_embed(frames, wm, wm_row=torch.zeros(n, dtype=torch.int32, device="cuda"), **kw)
    got = eng.svd_embed_copies(frames, wm, None, L=8, copies=1, soft=True, **kw)
    assert torch.equal(got[0][0], one) and torch.equal(got[3][0], eng.svd_detect_soft(one, 8, **kw))
    assert torch.equal(frames, before)


@pytest.mark.parametrize("scales", SCALES)
@pytest.mark.parametrize("blk", [4, 8])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", PLANAR_SHAPES)
def test_svd_planar_call(eng, shape, layout, blk, scales):
    import torch
    H, W, n = shape
    planes = planes_of(eng, shape, layout)
    before = planes.clone()
    wm = wm_of(H, W)
    kw = dict(scales=scales, blk=blk, layout=layout)
    tiles = int(eng.lib.ofmk_svd_count_tiles(H, W, blk))
    for C in COPIES:
        svd_case(lambda rows, **k: eng.svd_embed_copies_yuv420(planes, H, W, wm, rows, **k),
                 lambda copy, L: eng.svd_detect_soft_yuv420(copy, H, W, L, **kw), tiles, C, n, lengths(shape, PLANAR_SHAPES[:2]), **kw)
    assert torch.equal(planes, before)


def test_soft_sums_alone_through_the_c_abi(eng):
    """counts == bits == NULL: the engine always passes counts with L, so this goes through the library directly."""
    import torch
    from offmark import _hip
    H, W, n, C, L = 64, 96, 2, 3, 8
    frames, wm, rows = frames_of(n, H, W, 31), wm_of(H, W), rows_of(C, n)
    stream = _hip.current_stream()
    ref = eng.embed_detect_copies(frames, wm, rows, L, soft=True)
    out, soft = torch.empty_like(ref[0]), torch.full_like(ref[3], -77)
    ws = eng.copies_workspace(H, W, n, C)
    _hip.check(eng.lib.ofmk_embed_detect_copies_soft_rgb8(frames.data_ptr(), out.data_ptr(), C, n, H, W, wm.data_ptr(), N_WM, rows.data_ptr(),
                                                          20.0, L, None, None, soft.data_ptr(), 0, ws.data_ptr(), ws.numel(), stream, None))
    assert torch.equal(out, ref[0]) and torch.equal(soft, ref[3])
    ref = eng.svd_embed_copies(frames, wm, rows, L=L, soft=True)
    out, soft = torch.empty_like(ref[0]), torch.full_like(ref[3], -77)
    _hip.check(eng.lib.ofmk_svd_embed_copies_soft_rgb8(frames.data_ptr(), out.data_ptr(), C, n, H, W, wm.data_ptr(), N_WM, rows.data_ptr(),
                                                       _hip.scales3(15), 4, L, None, None, soft.data_ptr(), stream, None))
    assert torch.equal(out, ref[0]) and torch.equal(soft, ref[3])
    planes = eng.rgb_to_yuv420(frames, "nv12")
    ref = eng.svd_embed_copies_yuv420(planes, H, W, wm, rows, L=L, soft=True, layout="nv12")
    out, soft = torch.empty_like(ref[0]), torch.full_like(ref[3], -77)
    _hip.check(eng.lib.ofmk_svd_embed_copies_soft_yuv420(planes.data_ptr(), out.data_ptr(), _hip.YUV_NV12, C, n, H, W, wm.data_ptr(), N_WM,
                                                         rows.data_ptr(), _hip.scales3(15), 4, L, None, None, soft.data_ptr(), stream, None))
    assert torch.equal(out, ref[0]) and torch.equal(soft, ref[3])


# ---- independence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [8, 4096])
def test_dirty_destinations_and_a_second_call(eng, L):
    import torch
    C = 3
    H, W, n = 16, 24, 3
    frames, wm, rows = frames_of(n, H, W, 41), wm_of(H, W), rows_of(C, n)
    planes = eng.rgb_to_yuv420(frames, "i420")
    calls = {
        "dct": (lambda **k: eng.embed_detect_copies(frames, wm, rows, L, **k), (C, n, H, W, 3)),
        "svd": (lambda **k: eng.svd_embed_copies(frames, wm, rows, L=L, **k), (C, n, H, W, 3)),
        "planar": (lambda **k: eng.svd_embed_copies_yuv420(planes, H, W, wm, rows, L=L, **k), (C, n, H * W * 3 // 2)),
    }
    for name, (call, out_shape) in calls.items():
        ref = call(want_bits=True, soft=True)
        soft = torch.full((C, n, L), -0x5A5A5A5A5A, dtype=torch.int64, device="cuda")
        counts = torch.full((C, n, L), 0x5A5A5A5, dtype=torch.int32, device="cuda")
        out = torch.full(out_shape, 0xA5, dtype=torch.uint8, device="cuda")
        got = call(want_bits=True, soft=soft, counts=counts, out=out)
        assert got[0] is out and got[1] is counts and got[3] is soft and same(got, ref), name
        assert same(call(want_bits=True, soft=soft, counts=counts, out=out), ref), name          # into what the first call left


@pytest.mark.parametrize("shape", RGB_SHAPES)
def test_dct_results_do_not_depend_on_chunks_tile_order_or_route(eng, shape):
    from offmark import _hip
    from offmark.engine import DctEngine
    H, W, n = shape
    C = 3
    frames, wm, rows = frames_of(n, H, W, 51), wm_of(H, W), rows_of(C, n)
    ref = eng.embed_detect_copies(frames, wm, rows, 8, want_bits=True, soft=True)
    for chunk in (1, 2):
        assert same(DctEngine(chunk_frames=chunk).embed_detect_copies(frames, wm, rows, 8, want_bits=True, soft=True), ref), chunk
    for order in ("linear", "xcd"):
        assert same(DctEngine(tile_order=order).embed_detect_copies(frames, wm, rows, 8, want_bits=True, soft=True), ref), order
    for chunk in (None, 2):
        sep = DctEngine(chunk_frames=chunk, opts=_hip.Opts(_hip.F_SEPARATE_DETECT, 0, None))
        assert same(sep.embed_detect_copies(frames, wm, rows, 8, want_bits=True, soft=True), ref), chunk
    sep = DctEngine(chunk_frames=1, opts=_hip.Opts(_hip.F_SEPARATE_DETECT, 0, None))
    if shape in RGB_SHAPES[:2]:
        ref = eng.embed_detect_copies(frames, wm, rows, 4096, want_bits=True, soft=True)
        assert same(sep.embed_detect_copies(frames, wm, rows, 4096, want_bits=True, soft=True), ref)


@pytest.mark.parametrize("blk", [4, 8])
def test_no_channel_1_scale_gives_zeros(eng, blk):
    import torch
    H, W, n, C = 64, 96, 2, 3
    frames, wm, rows = frames_of(n, H, W, 61), wm_of(H, W), rows_of(C, n)
    kw = dict(scales=[15, 0, 0], blk=blk)
    ref = eng.svd_embed_copies(frames, wm, rows, L=8, want_bits=True, **kw)
    dirty = torch.full((C, n, 8), 99, dtype=torch.int64, device="cuda")
    got = eng.svd_embed_copies(frames, wm, rows, L=8, want_bits=True, soft=dirty, **kw)
    assert same(got[:3], ref) and not got[3].any() and not got[1].any()
    planes = eng.rgb_to_yuv420(frames, "nv12")
    ref = eng.svd_embed_copies_yuv420(planes, H, W, wm, rows, L=8, want_bits=True, layout="nv12", **kw)
    dirty.fill_(99)
    got = eng.svd_embed_copies_yuv420(planes, H, W, wm, rows, L=8, want_bits=True, soft=dirty, layout="nv12", **kw)
    assert same(got[:3], ref) and not got[3].any()


def test_launches_by_kind(eng):
    """n = 3 in chunks of 2.  DCT: one analysis and one fused launch per chunk, two small finalize launches per copy; DwtDctSvd
    blk 4: one launch for the whole call."""
    import torch
    from offmark import _hip
    from offmark.engine import DctEngine
    H, W, n, C = 64, 96, 3, 3
    frames, wm, rows = frames_of(n, H, W, 71), wm_of(H, W), rows_of(C, n)
    chunks = 2
    tm = _hip.Timing(256)
    e = DctEngine(chunk_frames=2, opts=tm.opts())
    ref = eng.embed_detect_copies(frames, wm, rows, 8, want_bits=True, soft=True)
    got = e.embed_detect_copies(frames, wm, rows, 8, want_bits=True, soft=True)
    torch.cuda.synchronize()
    kinds = tm.collect()
    assert same(got, ref)
    assert kinds["mark_fused"]["launches"] == chunks and kinds["analyze"]["launches"] == chunks
    assert kinds["mark"]["launches"] == 0 and kinds["finalize"]["launches"] == chunks * C * 2
    assert all(v["launches"] == 0 for k, v in kinds.items() if k not in ("mark_fused", "analyze", "finalize"))
    for call in (lambda: e.svd_embed_copies(frames, wm, rows, L=8, want_bits=True, soft=True),
                 lambda: e.svd_embed_copies_yuv420(e.rgb_to_yuv420(frames, "i420"), H, W, wm, rows, L=8, want_bits=True, soft=True)):
        call()
        torch.cuda.synchronize()
        kinds = tm.collect()
        assert kinds["svd"]["launches"] == 1 and kinds["svd"]["ms_total"] > 0
        assert all(v["launches"] == 0 for k, v in kinds.items() if k != "svd")
    tm.close()


@pytest.mark.parametrize("codec", ["dct", "svd", "svd_planar"])
def test_call_replays_from_a_graph(eng, codec):
    import torch
    H, W, n, C = 240, 320, 3, 3
    frames, wm, rows = frames_of(n, H, W, 81), wm_of(H, W), rows_of(C, n)
    planes = eng.rgb_to_yuv420(frames, "i420")
    call = {"dct": lambda **k: eng.embed_detect_copies(frames, wm, rows, 8, **k),
            "svd": lambda **k: eng.svd_embed_copies(frames, wm, rows, L=8, **k),
            "svd_planar": lambda **k: eng.svd_embed_copies_yuv420(planes, H, W, wm, rows, L=8, **k)}[codec]
    ref = call(soft=True)
    out, counts, soft = torch.empty_like(ref[0]), torch.empty_like(ref[1]), torch.empty_like(ref[3])
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        call(out=out, counts=counts, soft=soft)                     # warm-up on the capture stream
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            call(out=out, counts=counts, soft=soft)
    torch.cuda.synchronize()
    out.zero_()
    counts.zero_()
    soft.fill_(12345)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref[0]) and torch.equal(counts, ref[1]) and torch.equal(soft, ref[3])
    del graph
    import gc
    gc.collect()
    torch.cuda.synchronize()


def test_python_validation(eng):
    import torch
    H, W, n, C = 64, 96, 2, 3
    frames, wm, rows = frames_of(n, H, W, 5), wm_of(H, W), rows_of(C, n)
    planes = eng.rgb_to_yuv420(frames, "i420")
    calls = [lambda s: eng.embed_detect_copies(frames, wm, rows, 8, soft=s),
             lambda s: eng.svd_embed_copies(frames, wm, rows, L=8, soft=s),
             lambda s: eng.svd_embed_copies_yuv420(planes, H, W, wm, rows, L=8, soft=s)]
    for call in calls:
        with pytest.raises(ValueError):
            call(torch.empty((C, n, 4), dtype=torch.int64, device="cuda"))               # wrong shape
        with pytest.raises(ValueError):
            call(torch.empty((n, 8), dtype=torch.int64, device="cuda"))
        with pytest.raises(ValueError):
            call(torch.empty((C, n, 8), dtype=torch.int32, device="cuda"))               # wrong dtype
        with pytest.raises(ValueError):
            call(torch.empty((C, n, 16), dtype=torch.int64, device="cuda")[..., ::2])    # non-contiguous
    with pytest.raises(ValueError):
        eng.svd_embed_copies(frames, wm, rows, soft=True)                               # soft without a payload length


# ---- the fingerprint layer: per-(segment, copy) margins ---------------------------------------------------------------------------
class _PerCopy:
    """The encoder with the one-pass methods hidden: mark_segment_copies falls back to its per-copy loop."""

    def __init__(self, enc):
        self._enc = enc

    def encode_frames_u8(self, *a, **k):
        return self._enc.encode_frames_u8(*a, **k)

    def encode_planes_yuv420(self, *a, **k):
        return self._enc.encode_planes_yuv420(*a, **k)


def spy_on(obj, name, log):
    real = getattr(obj, name)

    def spy(*a, **k):
        log.append((name, k))
        return real(*a, **k)
    setattr(obj, name, spy)


FP_H, FP_W, FP_S, FP_F, FP_C = 240, 320, 2, 6, 3


def fingerprint_frames():
    """Segment 1: synthetic frames.  Segment 2: the same frames with block rows 0-15 (16 of 30) constant grey 128, so more than half
    of the units of every payload position are flat."""
    import torch
    one = frames_of(FP_F, FP_H, FP_W, 7000)
    two = one.clone()
    two[:, :128] = 128
    return torch.cat([one, two]).contiguous(), np.repeat(np.arange(1, FP_S + 1), FP_F)


def codec_pair(codec):
    if codec == "dct":
        from offmark.embed.dct_encoder import DctEncoder
        from offmark.extract.dct_decoder import DctDecoder
        return DctEncoder(), DctDecoder()
    from offmark.embed.dwt_dct_svd_encoder import DwtDctSvdEncoder
    from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder
    return DwtDctSvdEncoder(), DwtDctSvdDecoder()


def expected_margins(fp, copies, seg, soft_of):
    from offmark.generator.shuffler import Shuffler
    gen = Shuffler(key=0)
    units = (FP_H // 8) * (FP_W // 8)
    want = {}
    for c, copy in enumerate(copies):
        raw = {s: gen.generate_wm(fp.payload_for_segment(s, c), (FP_H * FP_W // 64,))[:8] for s in range(1, FP_S + 1)}
        per = fp.copy_margins(soft_of(copy.contiguous()), seg, raw, units)
        want.update({f"{s}_{c}": per[s] for s in per})
    return want


@pytest.mark.parametrize("planar", [False, True], ids=["rgb", "nv12"])
@pytest.mark.parametrize("codec", ["dct", "svd"])
def test_segment_margins(codec, planar):
    import torch
    from offmark import fingerprint as fp
    from offmark.engine import DctEngine
    frames, seg = fingerprint_frames()
    enc, dec = codec_pair(codec)
    log = []
    if planar:
        planes = DctEngine().rgb_to_yuv420(frames, "nv12")
        mark = lambda e, **k: fp.mark_segment_copies_yuv420(e, dec, planes, FP_H, FP_W, seg, FP_C, layout="nv12", **k)   # noqa: E731
        soft_of = lambda copy: dec.decode_soft_planes_yuv420(copy, FP_H, FP_W, 8, layout="nv12")                          # noqa: E731
        one_pass = "encode_verify_copies_planes_yuv420" if codec == "svd" else "encode_copies_planes_yuv420"
        soft_name, hard_name = "decode_soft_planes_yuv420", "decode_planes_yuv420"
    else:
        mark = lambda e, **k: fp.mark_segment_copies(e, dec, frames, seg, FP_C, **k)                                     # noqa: E731
        soft_of = lambda copy: dec.decode_soft_frames_u8(copy, 8)                                                        # noqa: E731
        one_pass = "encode_verify_copies_u8" if codec == "svd" else "encode_copies_u8"
        soft_name, hard_name = "decode_soft_frames_u8", "decode_frames_u8"
    fused_soft = not (codec == "dct" and planar)                     # the DCT codec on planes has no one-pass soft call
    want = expected_margins(fp, mark(enc)[0], seg, soft_of)
    for name in (one_pass, ):
        spy_on(enc, name, log)
    for name in (soft_name, hard_name):
        spy_on(dec, name, log)
    # margins=False: the sidecars and the calls of the call without the argument
    copies0, side0 = mark(enc)
    plain_log = list(log)
    del log[:]
    copies0b, side0b = mark(enc, margins=False)
    assert side0b == side0 and "segment_margins" not in side0 and [(n, sorted(k)) for n, k in log] == [(n, sorted(k)) for n, k in plain_log]
    assert all("soft" not in k for _, k in log) and all(n != soft_name for n, _ in log)
    # margins=True on the one-pass route
    del log[:]
    copies, side = mark(enc, margins=True)
    names = [n for n, _ in log]
    if fused_soft:
        assert soft_name not in names and names == [one_pass] and log[0][1].get("soft") is True
    else:
        assert names.count(soft_name) == FP_C
    assert set(side) == set(side0) | {"segment_margins"} and {k: v for k, v in side.items() if k != "segment_margins"} == side0
    assert side["segment_margins"] == want                           # float for float
    assert all(torch.equal(a, b) for a, b in zip(copies, copies0))
    # the per-copy fallback: equal copies, sidecars and margins, the soft sums from the decoder
    del log[:]
    copies_pc, side_pc = mark(_PerCopy(enc), margins=True)
    assert [n for n, _ in log].count(soft_name) == FP_C
    assert side_pc == side and all(torch.equal(a, b) for a, b in zip(copies_pc, copies))
    assert all(-1.0 <= m <= 1.0 for m in side["segment_margins"].values())
    if codec == "dct":
        # the flat blocks' C21 is exactly 0, where a 1-bit is lost (sign(0) = 0): no margin left in segment 2, yet the hard vote passes
        print("margins", side["segment_margins"], "failed", side["failed_segments"])
        first = [side["segment_margins"][f"1_{c}"] for c in range(FP_C)]
        second = [side["segment_margins"][f"2_{c}"] for c in range(FP_C)]
        assert side["failed_segments"] == []
        assert min(first) > 0 >= max(second), (first, second)


def test_margins_from_a_decoder_that_reads_differently():
    """A DctDecoder with another alpha does not read what the encoder's verify reads: counts and soft sums come from the decoder."""
    from offmark import fingerprint as fp
    from offmark.embed.dct_encoder import DctEncoder
    from offmark.extract.dct_decoder import DctDecoder
    frames, seg = fingerprint_frames()
    enc, other, log = DctEncoder(), DctDecoder(alpha=10), []
    spy_on(enc, "encode_copies_u8", log)
    spy_on(other, "decode_soft_frames_u8", log)
    copies, side = fp.mark_segment_copies(enc, other, frames, seg, FP_C, margins=True)
    assert [n for n, _ in log] == ["encode_copies_u8"] + ["decode_soft_frames_u8"] * FP_C and "soft" not in log[0][1]
    assert side["segment_margins"] == expected_margins(fp, copies, seg, lambda copy: other.decode_soft_frames_u8(copy, 8))
