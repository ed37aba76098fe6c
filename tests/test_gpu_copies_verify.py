"""GPU: the DCT codec's copies with the verify of every copy in the same pass (ofmk_embed_detect_copies_rgb8,
DctEngine.embed_detect_copies) against the single-copy calls, byte for byte and integer for integer: every copy equals embed with that
copy's watermark rows, its counts and bits equal embed_detect's and detect's of the written copy; nothing depends on the payload
length's path, on what the destinations held, on the chunking, the workspace size, the tile order or the fused / separate route;
the call is one fused launch per chunk; it replays from a captured graph; and the fingerprint layer takes its counts."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_WM = 5
SMALL = [(16, 24, 3), (64, 96, 2)]                         # 6 blocks: one ragged tile whose barriers mostly-invalid threads cross
SHAPES = SMALL + [(240, 320, 3), (250, 330, 3)]            # several tiles; unaligned rows, fringe and a ragged last tile


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


def same(got, ref):
    import torch
    return all((a is None and b is None) or torch.equal(a, b) for a, b in zip(got, ref))


_CASES = {}


def case(eng, shape, C=3, L=8):
    """One input and its result from the default engine, computed once per (shape, C, L) and never written to."""
    key = (shape, C, L)
    if key not in _CASES:
        H, W, n = shape
        frames = frames_of(n, H, W, 100 + H + C)
        wm, rows = wm_of(H, W), rows_of(C, n)
        _CASES[key] = (frames, wm, rows, eng.embed_detect_copies(frames, wm, rows, L, want_bits=True))
    return _CASES[key]


def check_against_single_copy_calls(eng, frames, wm, rows, L, C, got):
    import torch
    n, H, W, _ = frames.shape
    out, counts, bits = got
    assert tuple(out.shape) == (C, n, H, W, 3) and out.dtype == torch.uint8
    assert tuple(counts.shape) == (C, n, L) and counts.dtype == torch.int32
    assert tuple(bits.shape) == (C, n, H * W // 64) and bits.dtype == torch.uint8
    for c in range(C):
        assert torch.equal(out[c], eng.embed(frames, wm, wm_row=rows[c])), c
        _, rc, rb = eng.embed_detect(frames, wm, L, wm_row=rows[c], want_bits=True)
        assert torch.equal(counts[c], rc) and torch.equal(bits[c], rb), c
        dc, db = eng.detect(out[c].contiguous(), L, want_bits=True)
        assert torch.equal(counts[c], dc) and torch.equal(bits[c], db), c
    assert not bits[:, :, (H // 8) * (W // 8):].any()                    # entries past (H/8)*(W/8) are 0


@pytest.mark.parametrize("C", [1, 2, 3, 16])
@pytest.mark.parametrize("shape", SHAPES)
def test_copies_and_readouts_equal_the_single_copy_calls(eng, shape, C):
    import torch
    H, W, n = shape
    frames, wm, rows, got = case(eng, shape, C)
    before = frames.clone()
    check_against_single_copy_calls(eng, frames, wm, rows, 8, C, got)
    assert torch.equal(got[0], eng.embed_copies(frames, wm, rows))
    # no rows: copy c uses row c (clamped)
    got0 = eng.embed_detect_copies(frames, wm, None, 8, want_bits=True, copies=C)
    rows0 = torch.arange(C, dtype=torch.int32, device="cuda").clamp(max=N_WM - 1)[:, None].repeat(1, n).contiguous()
    check_against_single_copy_calls(eng, frames, wm, rows0, 8, C, got0)
    assert torch.equal(got0[0], eng.embed_copies(frames, wm, None, copies=C))
    assert torch.equal(frames, before)


def test_1080p_two_copies(eng):
    import torch
    shape = (1080, 1920, 2)
    frames, wm, rows, got = case(eng, shape, 2)
    before = frames.clone()
    check_against_single_copy_calls(eng, frames, wm, rows, 8, 2, got)
    assert torch.equal(got[0], eng.embed_copies(frames, wm, rows))
    assert torch.equal(frames, before)


# L = 5: not a power of two (no ballot path); L = 4096: above the LDS histogram, so global atomics (the small shapes are enough)
@pytest.mark.parametrize("shape,L", [(s, 5) for s in SMALL + [(250, 330, 3)]] + [(s, 4096) for s in SMALL])
def test_payload_length_paths(eng, shape, L):
    frames, wm, rows, got = case(eng, shape, 3, L)
    check_against_single_copy_calls(eng, frames, wm, rows, L, 3, got)


@pytest.mark.parametrize("L", [8, 4096])
@pytest.mark.parametrize("shape", [(16, 24, 3), (250, 330, 3)])
def test_dirty_destinations(eng, shape, L):
    import torch
    H, W, n = shape
    C = 3
    frames, wm, rows, ref = case(eng, shape, C, L)
    counts = torch.full((C, n, L), 0x5A5A5A5, dtype=torch.int32, device="cuda")
    out = torch.full((C, n, H, W, 3), 0xA5, dtype=torch.uint8, device="cuda")
    got = eng.embed_detect_copies(frames, wm, rows, L, out=out, want_bits=True, counts=counts)
    assert got[0] is out and got[1] is counts and same(got, ref)
    again = eng.embed_detect_copies(frames, wm, rows, L, out=out, want_bits=True, counts=counts)     # into what the first call left
    assert same(again, ref)
    only_counts = eng.embed_detect_copies(frames, wm, rows, L)
    assert only_counts[2] is None and same(only_counts[:2], ref[:2])


def test_bits_without_counts_through_the_c_abi(eng):
    """counts == NULL, caller-supplied dirty bits: the engine always passes counts, so this goes through the library directly."""
    import torch
    from offmark import _hip
    shape, C, L = (250, 330, 3), 3, 8
    H, W, n = shape
    frames, wm, rows, ref = case(eng, shape, C, L)
    out = torch.empty_like(ref[0])
    bits = torch.full_like(ref[2], 0xEE)
    ws = eng.copies_workspace(H, W, n, C)
    for _ in range(2):
        _hip.check(eng.lib.ofmk_embed_detect_copies_rgb8(frames.data_ptr(), out.data_ptr(), C, n, H, W, wm.data_ptr(), N_WM, rows.data_ptr(),
                                                         20.0, L, None, bits.data_ptr(), 0, ws.data_ptr(), ws.numel(),
                                                         _hip.current_stream(), None))
        assert torch.equal(out, ref[0]) and torch.equal(bits, ref[2])


@pytest.mark.parametrize("shape", SHAPES)
def test_results_do_not_depend_on_chunks_workspace_tile_order_or_route(eng, shape):
    from offmark import _hip
    from offmark.engine import DctEngine
    H, W, n = shape
    C = 3
    frames, wm, rows, ref = case(eng, shape, C)
    one = DctEngine(chunk_frames=1)                                 # chunks of one frame in a minimum workspace
    got = one.embed_detect_copies(frames, wm, rows, 8, want_bits=True)
    assert one.copies_workspace(H, W, 1, C).numel() == one.lib.ofmk_copies_workspace_bytes(1, C, H, W)
    assert same(got, ref)
    two = DctEngine(chunk_frames=2)                                 # n = 3: a ragged last chunk, copy-major offsets across chunks
    assert same(two.embed_detect_copies(frames, wm, rows, 8, want_bits=True), ref)
    for order in ("linear", "xcd"):
        assert same(DctEngine(tile_order=order).embed_detect_copies(frames, wm, rows, 8, want_bits=True), ref), order
    for chunk in (None, 2):
        sep = DctEngine(chunk_frames=chunk, opts=_hip.Opts(_hip.F_SEPARATE_DETECT, 0, None))
        assert same(sep.embed_detect_copies(frames, wm, rows, 8, want_bits=True), ref), chunk


def test_separate_route_with_long_payload(eng):
    from offmark import _hip
    from offmark.engine import DctEngine
    frames, wm, rows, ref = case(eng, (64, 96, 2), 3, 4096)
    sep = DctEngine(chunk_frames=1, opts=_hip.Opts(_hip.F_SEPARATE_DETECT, 0, None))
    assert same(sep.embed_detect_copies(frames, wm, rows, 4096, want_bits=True), ref)


def test_one_fused_launch_per_chunk(eng):
    """What tells a fused pass from a host-side loop over the single-copy call: the launches, by kind."""
    import torch
    from offmark import _hip
    from offmark.engine import DctEngine
    shape, C = (64, 96, 3), 3
    H, W, n = shape
    frames, wm, rows, ref = case(eng, shape, C)
    chunks = 2                                                      # n = 3 in chunks of 2
    tm = _hip.Timing(256)
    e = DctEngine(chunk_frames=2, opts=tm.opts())
    got = e.embed_detect_copies(frames, wm, rows, 8, want_bits=True)
    torch.cuda.synchronize()
    kinds = tm.collect()
    assert same(got, ref)
    assert kinds["mark_fused"]["launches"] == chunks and kinds["mark_fused"]["ms_total"] > 0       # kind 3
    assert kinds["analyze"]["launches"] == chunks                                                  # kind 0
    assert kinds["mark"]["launches"] == 0                                                          # kind 2
    assert kinds["finalize"]["launches"] == chunks * C                                             # kind 1: one small launch per copy
    assert all(v["launches"] == 0 for k, v in kinds.items() if k not in ("mark_fused", "analyze", "finalize"))
    e = DctEngine(chunk_frames=2, opts=tm.opts(_hip.F_SEPARATE_DETECT))
    got = e.embed_detect_copies(frames, wm, rows, 8, want_bits=True)
    torch.cuda.synchronize()
    kinds = tm.collect()
    tm.close()
    assert same(got, ref)
    assert kinds["mark_fused"]["launches"] == 0
    assert kinds["analyze"]["launches"] == chunks * (1 + C)
    assert kinds["mark"]["launches"] == chunks and kinds["finalize"]["launches"] == chunks * C


def test_call_replays_from_a_graph(eng):
    import torch
    shape, C = (240, 320, 3), 3
    frames, wm, rows, ref = case(eng, shape, C)
    out = torch.empty_like(ref[0])
    counts = torch.empty_like(ref[1])
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng.embed_detect_copies(frames, wm, rows, 8, out=out, counts=counts)         # warm-up on the capture stream
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            eng.embed_detect_copies(frames, wm, rows, 8, out=out, counts=counts)
    torch.cuda.synchronize()
    out.zero_()
    counts.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref[0]) and torch.equal(counts, ref[1])
    del graph
    import gc
    gc.collect()
    torch.cuda.synchronize()


class _PerCopy:
    """The encoder with the one-pass methods hidden: mark_segment_copies falls back to its per-copy loop."""

    def __init__(self, enc):
        self._enc = enc

    def encode_frames_u8(self, *a, **k):
        return self._enc.encode_frames_u8(*a, **k)


def spy_on(obj, name, log):
    real = getattr(obj, name)

    def spy(*a, **k):
        log.append((name, k))
        return real(*a, **k)
    setattr(obj, name, spy)


def test_mark_segment_copies_takes_the_counts_of_the_pass():
    import torch
    from offmark import fingerprint as fp
    from offmark.embed.dct_encoder import DctEncoder
    from offmark.extract.dct_decoder import DctDecoder
    H, W, S, C, F = 240, 320, 4, 3, 6
    frames = frames_of(S * F, H, W, 6000)
    seg = np.repeat(np.arange(1, S + 1), F)
    enc, dec, log = DctEncoder(), DctDecoder(), []
    spy_on(enc, "encode_copies_u8", log)
    spy_on(dec, "decode_frames_u8", log)
    copies, side = fp.mark_segment_copies(enc, dec, frames, seg, C)
    assert [name for name, _ in log] == ["encode_copies_u8"] and log[0][1].get("verify_len") == 8
    ref_copies, ref_side = fp.mark_segment_copies(_PerCopy(enc), dec, frames, seg, C)
    assert [name for name, _ in log] == ["encode_copies_u8"] + ["decode_frames_u8"] * C
    assert side == ref_side and not side["failed_segments"]
    assert len(copies) == C and all(torch.equal(a, b) for a, b in zip(copies, ref_copies))
    # a decoder that does not read what the encoder's verify reads is asked, as before
    other, log2 = DctDecoder(alpha=10), []
    del log[:]
    spy_on(other, "decode_frames_u8", log2)
    copies10, _ = fp.mark_segment_copies(enc, other, frames, seg, C)
    assert [name for name, _ in log] == ["encode_copies_u8"] and log[0][1].get("verify_len") is None
    assert [name for name, _ in log2] == ["decode_frames_u8"] * C
    assert all(torch.equal(a, b) for a, b in zip(copies10, ref_copies))


def test_python_validation(eng):
    import torch
    H, W, n = 64, 96, 2
    frames = frames_of(n, H, W, 5)
    wm, rows = wm_of(H, W), rows_of(3, n)
    call = eng.embed_detect_copies
    with pytest.raises(ValueError):
        call(frames, wm, rows_of(3, n + 1), 8)                                  # wrong wm_rows shape
    with pytest.raises(ValueError):
        call(frames, wm, rows[0], 8)                                            # one-dimensional rows
    with pytest.raises(ValueError):
        call(frames, wm, np.full((2, n), N_WM, np.int32), 8)                    # host rows out of range
    with pytest.raises(ValueError):
        call(frames, wm, rows, 8, out=torch.empty((2, n, H, W, 3), dtype=torch.uint8, device="cuda"))
    wide = torch.empty((3, n, H, W, 6), dtype=torch.uint8, device="cuda")[..., :3]
    with pytest.raises(ValueError):
        call(frames, wm, rows, 8, out=wide)                                     # non-contiguous out
    with pytest.raises(ValueError):
        call(frames, wm, rows, 8, counts=torch.empty((3, n, 4), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        call(frames, wm, rows, 8, counts=torch.empty((n, 8), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        call(frames, wm, None, 8, copies=17)
