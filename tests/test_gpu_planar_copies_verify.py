"""GPU: the DCT codec's copies on 4:2:0 planes with the verify of every copy in the same pass, hard and soft
(ofmk_embed_detect_copies_yuv420 / ofmk_embed_detect_copies_soft_yuv420, DctEngine.embed_detect_copies_yuv420) against the calls
that were there before, byte for byte and integer for integer (every comparison is torch.equal): the copies equal
embed_copies_yuv420's, every copy's counts and bits equal detect_yuv420's of the written copy and embed_detect_yuv420's with that
copy's rows, its soft sums equal detect_soft_yuv420's of the written copy; whichever of its two marked forms the copies of a block
take; nothing depends on the chunking, the workspace size, the route or what the destinations held; the call is one analyze and one
mark launch per chunk; it replays from a captured graph; and the fingerprint layer takes its counts and soft sums when asked to."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_WM = 5
# one block in a ragged tile; 15 blocks; 357 blocks = two workgroups, the last one partial, and n = 3 against chunks of 2
TINY, SMALL, TWO_TILES = (8, 8, 1), (24, 40, 2), (136, 168, 3)
SHAPES = [TINY, SMALL, TWO_TILES]
LAYOUTS = ["i420", "nv12"]


@pytest.fixture(scope="module")
def eng():
    import torch
    from offmark.engine import DctEngine
    torch.cuda.set_device(0)
    return DctEngine()


_PLANES = {}


def planes_of(eng, shape, layout, kind="synthetic"):
    """Input planes, made once per (shape, layout, kind) and never written to.  kind: synthetic frames, or a constant RGB value."""
    import torch
    from offmark.synthetic import synthetic_frames
    key = (shape, layout, kind)
    if key not in _PLANES:
        H, W, n = shape
        rgb = synthetic_frames(n, H, W, seed=100 + H) if kind == "synthetic" \
            else torch.full((n, H, W, 3), int(kind), dtype=torch.uint8, device="cuda")
        _PLANES[key] = eng.rgb_to_yuv420(rgb, layout)
    return _PLANES[key]


def wm_of(H, W, table="random", seed=7):
    """[N_WM, N] watermark table.  "equal": every row the same (no block needs its second form); "first": row 0 all ones and the
    others all zeros (copy 0 alone takes the form of bit 1)."""
    import torch
    N = H * W // 64
    bits = np.random.default_rng(seed).integers(0, 2, (N_WM, N), dtype=np.uint8)
    if table == "equal":
        bits[:] = bits[0]
    elif table == "first":
        bits[:] = 0
        bits[0] = 1
    return torch.from_numpy(bits).cuda()


def rows_of(C, n, seed=11):
    """[C, n] device rows that vary per frame, out-of-range entries included (the kernels clamp them into [0, N_WM))."""
    import torch
    r = np.random.default_rng(seed).integers(-2, N_WM + 3, (C, n)).astype(np.int32)
    return torch.from_numpy(r).cuda()


def same(got, ref):
    import torch
    return len(got) == len(ref) and all((a is None and b is None) or torch.equal(a, b) for a, b in zip(got, ref))


_CASES = {}


def case(eng, shape, layout, C=3, L=8, table="random", kind="synthetic"):
    """One input and its (out, counts, bits, soft) from the default engine, computed once per key and never written to."""
    key = (shape, layout, C, L, table, kind)
    if key not in _CASES:
        H, W, n = shape
        planes = planes_of(eng, shape, layout, kind)
        wm, rows = wm_of(H, W, table), rows_of(C, n)
        _CASES[key] = (planes, wm, rows, eng.embed_detect_copies_yuv420(planes, H, W, wm, rows, L, want_bits=True, layout=layout, soft=True))
    return _CASES[key]


def check_against_existing_calls(eng, planes, shape, layout, wm, rows, L, C, got):
    import torch
    H, W, n = shape
    out, counts, bits, soft = got
    assert tuple(out.shape) == (C, n, H * W * 3 // 2) and out.dtype == torch.uint8
    assert tuple(counts.shape) == (C, n, L) and counts.dtype == torch.int32
    assert tuple(bits.shape) == (C, n, H * W // 64) and bits.dtype == torch.uint8
    assert tuple(soft.shape) == (C, n, L) and soft.dtype == torch.int64
    assert torch.equal(out, eng.embed_copies_yuv420(planes, H, W, wm, rows, layout=layout))
    for c in range(C):
        dc, db = eng.detect_yuv420(out[c], H, W, L, want_bits=True, layout=layout)
        assert torch.equal(counts[c], dc) and torch.equal(bits[c], db), c
        eo, ec, eb = eng.embed_detect_yuv420(planes, H, W, wm, L, wm_row=rows[c], want_bits=True, layout=layout)
        assert torch.equal(out[c], eo) and torch.equal(counts[c], ec) and torch.equal(bits[c], eb), c
        assert torch.equal(soft[c], eng.detect_soft_yuv420(out[c], H, W, L, layout=layout)), c


def row_c(C, n):
    """What wm_rows=None means: copy c uses row c (clamped) for every frame."""
    import torch
    return torch.arange(C, dtype=torch.int32, device="cuda").clamp(max=N_WM - 1)[:, None].repeat(1, n).contiguous()


def raw_call(eng, planes, shape, layout, wm, rows, L, C, want=("counts", "bits", "soft"), chunk=0, ws_frames=None, flags=0, fill=None):
    """Through the C ABI: any subset of the outputs (NULL for the others), any workspace size.  Returns (out, counts, bits, soft)."""
    import torch
    from offmark import _hip
    H, W, n = shape
    N = H * W // 64
    mk = lambda sh, dt: (torch.empty(sh, dtype=dt, device="cuda") if fill is None                                     # noqa: E731
                         else torch.full(sh, fill, dtype=dt, device="cuda"))
    out = mk((C, n, H * W * 3 // 2), torch.uint8)
    counts = mk((C, n, L), torch.int32) if "counts" in want else None
    bits = mk((C, n, N), torch.uint8) if "bits" in want else None
    soft = mk((C, n, L), torch.int64) if "soft" in want else None
    nbytes = eng.lib.ofmk_copies_workspace_bytes(ws_frames or n, C, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    opts = _hip.Opts(flags, 0, None)
    head = (planes.data_ptr(), out.data_ptr(), eng._layout(layout), C, n, H, W, wm.data_ptr(), wm.shape[0], _hip.ptr(rows), 20.0, L,
            _hip.ptr(counts), _hip.ptr(bits))
    tail = (chunk, ws.data_ptr(), ws.numel(), _hip.current_stream(), _hip.opts_ref(opts))
    if "soft" in want:
        _hip.check(eng.lib.ofmk_embed_detect_copies_soft_yuv420(*head, soft.data_ptr(), *tail))
    else:
        _hip.check(eng.lib.ofmk_embed_detect_copies_yuv420(*head, *tail))
    torch.cuda.synchronize()                                          # the workspace goes out of scope
    return out, counts, bits, soft


# ---- 1. against the calls that exist without this one --------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [8, 5])
@pytest.mark.parametrize("C", [1, 3, 16])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_copies_and_readouts_equal_the_existing_calls(eng, shape, layout, C, L):
    import torch
    H, W, n = shape
    planes, wm, rows, got = case(eng, shape, layout, C, L)
    before = planes.clone()
    check_against_existing_calls(eng, planes, shape, layout, wm, rows, L, C, got)
    hard = eng.embed_detect_copies_yuv420(planes, H, W, wm, rows, L, want_bits=True, layout=layout)       # the hard call alone
    assert len(hard) == 3 and same(hard, got[:3])
    no_bits = eng.embed_detect_copies_yuv420(planes, H, W, wm, rows, L, layout=layout)
    assert no_bits[2] is None and same(no_bits[:2], got[:2])
    # no rows: copy c uses row c (clamped)
    got0 = eng.embed_detect_copies_yuv420(planes, H, W, wm, None, L, want_bits=True, copies=C, layout=layout, soft=True)
    check_against_existing_calls(eng, planes, shape, layout, wm, row_c(C, n), L, C, got0)
    assert torch.equal(got0[0], eng.embed_copies_yuv420(planes, H, W, wm, None, copies=C, layout=layout))
    assert torch.equal(planes, before)


# L = 4096: above finalize's LDS histogram, so global atomics
@pytest.mark.parametrize("C", [1, 3, 16])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [TINY, SMALL])
def test_long_payload(eng, shape, layout, C):
    planes, wm, rows, got = case(eng, shape, layout, C, 4096)
    check_against_existing_calls(eng, planes, shape, layout, wm, rows, 4096, C, got)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_subsets_of_the_outputs_through_the_c_abi(eng, shape, layout):
    """The soft sums alone (counts and bits NULL), bits without counts, counts without bits: the engine always passes counts."""
    C, L = 3, 8
    planes, wm, rows, ref = case(eng, shape, layout, C, L)
    out, counts, bits, soft = raw_call(eng, planes, shape, layout, wm, rows, L, C, want=("soft",), fill=0x5A)
    assert counts is None and bits is None and same((out, soft), (ref[0], ref[3]))
    out, counts, bits, soft = raw_call(eng, planes, shape, layout, wm, rows, L, C, want=("bits",), fill=0x5A)
    assert same((out, bits), (ref[0], ref[2]))
    out, counts, bits, soft = raw_call(eng, planes, shape, layout, wm, rows, L, C, want=("counts", "soft"), fill=0x5A)
    assert same((out, counts, soft), (ref[0], ref[1], ref[3]))


# ---- 2. the two marked forms of a block ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["equal", "first"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [SMALL, TWO_TILES])
def test_tables_that_decide_which_forms_a_block_needs(eng, shape, layout, table):
    """Every row equal: the second pass is skipped everywhere.  Row 0 all ones, the others zeros, copy c using row c: copy 0 alone
    takes the form of bit 1 and every block needs both.  (The random table of the other tests mixes the cases lane by lane.)"""
    H, W, n = shape
    C, L = 3, 8
    planes, wm = planes_of(eng, shape, layout), wm_of(H, W, table)
    got = eng.embed_detect_copies_yuv420(planes, H, W, wm, None, L, want_bits=True, copies=C, layout=layout, soft=True)
    check_against_existing_calls(eng, planes, shape, layout, wm, row_c(C, n), L, C, got)
    rows = rows_of(C, n)
    got = eng.embed_detect_copies_yuv420(planes, H, W, wm, rows, L, want_bits=True, layout=layout, soft=True)
    check_against_existing_calls(eng, planes, shape, layout, wm, rows, L, C, got)


@pytest.mark.parametrize("value", [128, 0, 255], ids=["grey", "black", "white"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_constant_frames(eng, layout, value):
    """Constant grey: C21 is exactly 0, a 1-bit is lost and both changes are 0; black and white: the clipping ends of the range."""
    for table in ("random", "first"):
        planes, wm, rows, got = case(eng, SMALL, layout, 3, 8, table, kind=value)
        check_against_existing_calls(eng, planes, SMALL, layout, wm, rows, 8, 3, got)


# ---- 3. what the results must not depend on --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_results_do_not_depend_on_chunks_workspace_or_route(eng, shape, layout):
    from offmark import _hip
    from offmark.engine import DctEngine
    H, W, n = shape
    C, L = 3, 8
    planes, wm, rows, ref = case(eng, shape, layout, C, L)
    call = lambda e: e.embed_detect_copies_yuv420(planes, H, W, wm, rows, L, want_bits=True, layout=layout, soft=True)   # noqa: E731
    one = DctEngine(chunk_frames=1)                                 # chunks of one frame in a minimum workspace
    got = call(one)
    assert one.copies_workspace(H, W, 1, C).numel() == one.lib.ofmk_copies_workspace_bytes(1, C, H, W)
    assert same(got, ref)
    assert same(call(DctEngine(chunk_frames=2)), ref)               # n = 3: a ragged last chunk, copy-major offsets across chunks
    # the minimal workspace without a chunk size (the call chunks itself), and one far larger than the batch
    assert same(raw_call(eng, planes, shape, layout, wm, rows, L, C, ws_frames=1), ref)
    assert same(raw_call(eng, planes, shape, layout, wm, rows, L, C, ws_frames=64), ref)
    for chunk in (None, 1, 2):
        sep = DctEngine(chunk_frames=chunk, opts=_hip.Opts(_hip.F_SEPARATE_DETECT, 0, None))
        assert same(call(sep), ref), chunk
        assert same(sep.embed_detect_copies_yuv420(planes, H, W, wm, rows, L, want_bits=True, layout=layout), ref[:3]), chunk
    assert same(raw_call(eng, planes, shape, layout, wm, rows, L, C, want=("soft",), flags=_hip.F_SEPARATE_DETECT)[::3], ref[::3])


@pytest.mark.parametrize("shape,layout,L", [(SMALL, "i420", 8), (TWO_TILES, "nv12", 8), (SMALL, "nv12", 4096)])
def test_dirty_destinations_and_a_second_call(eng, shape, layout, L):
    import torch
    H, W, n = shape
    C = 3
    planes, wm, rows, ref = case(eng, shape, layout, C, L)
    counts = torch.full((C, n, L), 0x5A5A5A5, dtype=torch.int32, device="cuda")
    soft = torch.full((C, n, L), -0x123456789, dtype=torch.int64, device="cuda")
    out = torch.full((C, n, H * W * 3 // 2), 0xA5, dtype=torch.uint8, device="cuda")
    call = lambda: eng.embed_detect_copies_yuv420(planes, H, W, wm, rows, L, out=out, want_bits=True, counts=counts, layout=layout,   # noqa: E731
                                                  soft=soft)
    got = call()
    assert got[0] is out and got[1] is counts and got[3] is soft and same(got, ref)
    assert same(call(), ref)                                        # into what the first call left


# ---- 4. launches, by kind --------------------------------------------------------------------------------------------------------------
def test_one_analyze_and_one_mark_launch_per_chunk(eng):
    """What tells the one-pass call from a host-side loop over the single-copy call: the launches, by kind."""
    import torch
    from offmark import _hip
    from offmark.engine import DctEngine
    shape, layout, C, L = (64, 96, 3), "nv12", 3, 8
    H, W, n = shape
    planes, wm, rows, ref = case(eng, shape, layout, C, L)
    chunks = 2                                                      # n = 3 in chunks of 2
    tm = _hip.Timing(256)
    e = DctEngine(chunk_frames=2, opts=tm.opts())

    def kinds_of(run):
        got = run()
        torch.cuda.synchronize()
        return got, {k: v["launches"] for k, v in tm.collect().items()}

    def expect(kinds, finalize):
        assert kinds["planar_analyze"] == chunks and kinds["planar_mark"] == chunks        # kinds 5 and 6
        assert kinds["finalize"] == finalize                                               # kind 1
        assert all(v == 0 for k, v in kinds.items() if k not in ("planar_analyze", "planar_mark", "finalize")), kinds

    got, kinds = kinds_of(lambda: e.embed_detect_copies_yuv420(planes, H, W, wm, rows, L, want_bits=True, layout=layout))
    assert same(got, ref[:3])
    expect(kinds, chunks * C)                                       # hard only: one small launch per copy
    got, kinds = kinds_of(lambda: e.embed_detect_copies_yuv420(planes, H, W, wm, rows, L, want_bits=True, layout=layout, soft=True))
    assert same(got, ref)
    expect(kinds, chunks * C * 2)                                   # hard + soft: two per copy
    out = torch.empty_like(ref[0])
    soft = torch.empty_like(ref[3])
    ws = e.copies_workspace(H, W, 2, C)
    opts = tm.opts()

    def soft_alone():
        _hip.check(e.lib.ofmk_embed_detect_copies_soft_yuv420(planes.data_ptr(), out.data_ptr(), e._layout(layout), C, n, H, W, wm.data_ptr(),
                                                              N_WM, rows.data_ptr(), 20.0, L, None, None, soft.data_ptr(), 2, ws.data_ptr(),
                                                              ws.numel(), _hip.current_stream(), _hip.opts_ref(opts)))
        return out, soft
    got, kinds = kinds_of(soft_alone)
    assert same(got, ref[::3])
    expect(kinds, chunks * C)                                       # soft alone: one per copy
    tm.close()


# ---- 5. graph capture --------------------------------------------------------------------------------------------------------------------
def test_soft_call_replays_from_a_graph(eng):
    import torch
    shape, layout, C, L = TWO_TILES, "nv12", 3, 8
    H, W, n = shape
    planes, wm, rows, ref = case(eng, shape, layout, C, L)
    out, counts, soft = torch.empty_like(ref[0]), torch.empty_like(ref[1]), torch.empty_like(ref[3])
    call = lambda: eng.embed_detect_copies_yuv420(planes, H, W, wm, rows, L, out=out, counts=counts, layout=layout, soft=soft)   # noqa: E731
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        call()                                                      # warm-up on the capture stream (sizes the workspace)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            call()
    torch.cuda.synchronize()
    out.zero_()
    counts.zero_()
    soft.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref[0]) and torch.equal(counts, ref[1]) and torch.equal(soft, ref[3])
    del graph
    import gc
    gc.collect()
    torch.cuda.synchronize()


# ---- 6. Python validation ----------------------------------------------------------------------------------------------------------------
def test_python_validation(eng):
    import torch
    from offmark.embed.dct_encoder import DctEncoder
    H, W, n, C = 24, 40, 2, 3
    planes, wm, rows = planes_of(eng, SMALL, "i420"), wm_of(H, W), rows_of(C, n)
    call = lambda **k: eng.embed_detect_copies_yuv420(planes, H, W, wm, rows, 8, **k)      # noqa: E731
    with pytest.raises(ValueError):
        call(soft=torch.empty((C, n, 4), dtype=torch.int64, device="cuda"))               # wrong shape
    with pytest.raises(ValueError):
        call(soft=torch.empty((n, 8), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        call(soft=torch.empty((C, n, 8), dtype=torch.int32, device="cuda"))               # wrong dtype
    with pytest.raises(ValueError):
        call(soft=torch.empty((C, n, 16), dtype=torch.int64, device="cuda")[..., ::2])    # non-contiguous
    with pytest.raises(ValueError):
        call(layout="yv12")
    with pytest.raises(ValueError):
        call(out=torch.empty((2, n, H * W * 3 // 2), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        call(counts=torch.empty((n, 8), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        eng.embed_detect_copies_yuv420(planes, H, W, wm, None, 8, copies=17)
    with pytest.raises(ValueError):
        eng.embed_detect_copies_yuv420(planes, H, W, wm, rows_of(C, n + 1), 8)
    with pytest.raises(ValueError):
        eng.embed_detect_copies_yuv420(planes[:, :-8], H, W, wm, rows, 8)
    with pytest.raises(ValueError):
        DctEncoder().encode_copies_planes_yuv420(planes, H, W, rows, wm, soft=True)      # soft without verify_len


def test_encoder_returns_what_the_engine_returns(eng):
    import torch
    from offmark.embed.dct_encoder import DctEncoder
    H, W, n = SMALL
    planes, wm, rows, ref = case(eng, SMALL, "nv12", 3, 8)
    enc = DctEncoder()
    plain = enc.encode_copies_planes_yuv420(planes, H, W, rows, wm, layout="nv12")
    assert isinstance(plain, torch.Tensor) and torch.equal(plain, ref[0])                # without verify_len: unchanged
    assert same(enc.encode_copies_planes_yuv420(planes, H, W, rows, wm, layout="nv12", verify_len=8), ref[:2])
    assert same(enc.encode_copies_planes_yuv420(planes, H, W, rows, wm, layout="nv12", verify_len=8, soft=True), (ref[0], ref[1], ref[3]))


# ---- 7. the fingerprint layer --------------------------------------------------------------------------------------------------------
FP_H, FP_W, FP_S, FP_F, FP_C = 240, 320, 2, 6, 3
ENC_NAME = "encode_copies_planes_yuv420"
DEC_NAMES = ("decode_planes_yuv420", "decode_soft_planes_yuv420")


def fingerprint_planes(eng):
    """Segment 1: synthetic frames.  Segment 2: the same frames with block rows 0-15 (16 of 30) constant grey 128, so more than half
    of the units of every payload position are flat."""
    import torch
    from offmark.synthetic import synthetic_frames
    one = synthetic_frames(FP_F, FP_H, FP_W, seed=7000)
    two = one.clone()
    two[:, :128] = 128
    return eng.rgb_to_yuv420(torch.cat([one, two]).contiguous(), "nv12"), np.repeat(np.arange(1, FP_S + 1), FP_F)


def spy_on(obj, name, log):
    real = getattr(obj, name)

    def spy(*a, **k):
        log.append((name, k))
        return real(*a, **k)
    setattr(obj, name, spy)


def test_mark_segment_copies_yuv420_one_pass_verify(eng):
    import torch
    from offmark import fingerprint as fp
    from offmark.embed.dct_encoder import DctEncoder
    from offmark.extract.dct_decoder import DctDecoder
    planes, seg = fingerprint_planes(eng)
    enc, dec, log = DctEncoder(), DctDecoder(), []
    spy_on(enc, ENC_NAME, log)
    for name in DEC_NAMES:
        spy_on(dec, name, log)
    mark = lambda d=dec, **k: fp.mark_segment_copies_yuv420(enc, d, planes, FP_H, FP_W, seg, FP_C, layout="nv12", **k)   # noqa: E731
    names = lambda: [n for n, _ in log]                                                                                # noqa: E731
    # the default, and one_pass_verify=False: the call log of before (the decoder reads every copy, twice with margins)
    copies0, side0 = mark()
    assert names() == [ENC_NAME] + [DEC_NAMES[0]] * FP_C and "verify_len" not in log[0][1] and "soft" not in log[0][1]
    del log[:]
    copies0m, side0m = mark(margins=True, one_pass_verify=False)
    assert names()[0] == ENC_NAME and "verify_len" not in log[0][1] and "soft" not in log[0][1]
    assert sorted(names()[1:]) == [DEC_NAMES[0]] * FP_C + [DEC_NAMES[1]] * FP_C
    # one_pass_verify=True: one encoder call with the verify, no decoder call; equal copies and sidecars
    del log[:]
    copies1, side1 = mark(one_pass_verify=True)
    assert names() == [ENC_NAME] and log[0][1].get("verify_len") == 8 and "soft" not in log[0][1]
    assert side1 == side0 and "segment_margins" not in side1
    assert all(torch.equal(a, b) for a, b in zip(copies1, copies0))
    # every copy's vote from the one-pass counts equals its payload, the half-flat second segment included
    assert side1["failed_segments"] == []
    # with margins: the soft sums of the same call; margins equal float for float
    del log[:]
    copies1m, side1m = mark(margins=True, one_pass_verify=True)
    assert names() == [ENC_NAME] and log[0][1].get("verify_len") == 8 and log[0][1].get("soft") is True
    assert side1m == side0m and set(side1m["segment_margins"]) == {f"{s}_{c}" for s in (1, 2) for c in range(FP_C)}
    assert {k: v for k, v in side1m.items() if k != "segment_margins"} == side0
    assert all(torch.equal(a, b) for a, b in zip(copies1m, copies0))
    # a decoder that does not read what the encoder's verify reads is asked, as before
    other, log2 = DctDecoder(alpha=10), []
    for name in DEC_NAMES:
        spy_on(other, name, log2)
    del log[:]
    copies10, side10 = mark(other, margins=True, one_pass_verify=True)
    assert names() == [ENC_NAME] and "verify_len" not in log[0][1] and "soft" not in log[0][1]
    assert sorted(n for n, _ in log2) == [DEC_NAMES[0]] * FP_C + [DEC_NAMES[1]] * FP_C
    assert all(torch.equal(a, b) for a, b in zip(copies10, copies0))


def test_one_pass_verify_changes_nothing_for_the_other_codec(eng):
    """DwtDctSvd takes its one-pass verify with or without the keyword."""
    import torch
    from offmark import fingerprint as fp
    from offmark.embed.dwt_dct_svd_encoder import DwtDctSvdEncoder
    from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder
    planes, seg = fingerprint_planes(eng)
    enc, dec, log = DwtDctSvdEncoder(), DwtDctSvdDecoder(), []
    spy_on(enc, "encode_verify_copies_planes_yuv420", log)
    for name in DEC_NAMES:
        spy_on(dec, name, log)
    a = fp.mark_segment_copies_yuv420(enc, dec, planes, FP_H, FP_W, seg, FP_C, layout="nv12", margins=True)
    b = fp.mark_segment_copies_yuv420(enc, dec, planes, FP_H, FP_W, seg, FP_C, layout="nv12", margins=True, one_pass_verify=True)
    assert [n for n, _ in log] == ["encode_verify_copies_planes_yuv420"] * 2 and log[0][1] == log[1][1]
    assert a[1] == b[1] and all(torch.equal(x, y) for x, y in zip(a[0], b[0]))
