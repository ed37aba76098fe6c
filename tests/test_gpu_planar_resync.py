"""GPU: block-grid resync of cropped 4:2:0 planes, both codecs, I420 and NV12 (engine.svd_sync_scores_yuv420 /
svd_detect_soft_window_yuv420 / sync_scores_yuv420 / detect_soft_window_yuv420, offmark.resync.read_cropped_leak_yuv420; build
extensions, not reference semantics).

Device against device is exact, integer for integer, nothing masked out, output buffers pre-filled with garbage: the dense search
against the EXISTING planar soft read-out of every even sub(py, px) -- the frame's sub-planes for the pixel window
[py : py + 8r, px : px + 8c] -- with the odd and unit-less entries exactly 0, and the window read-out against the per-unit planar
read-out of sub(py, px) regrouped on the host.  The statement over the oracle is tests/test_planar_resync_statement.py's."""
import numpy as np
import pytest

import offmark_oracle as orc
import _planar_resync as pr

pytestmark = pytest.mark.gpu

LAYOUTS = ("i420", "nv12")


@pytest.fixture(scope="module")
def eng():
    import torch
    from offmark.engine import DctEngine
    torch.cuda.set_device(0)
    return DctEngine()


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()             # a copy: the shared references are read-only


def garbage(n, L):
    """The output buffer a call gets holds anything: the library clears it."""
    import torch
    return torch.full((n, L), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")


def split(dev, H, W, layout):
    n = dev.shape[0]
    y = dev[:, :H * W].reshape(n, H, W)
    if layout == "i420":
        q = H * W // 4
        return y, dev[:, H * W:H * W + q].reshape(n, H // 2, W // 2), dev[:, H * W + q:].reshape(n, H // 2, W // 2)
    uv = dev[:, H * W:].reshape(n, H // 2, W // 2, 2)
    return y, uv[..., 0], uv[..., 1]


def device_crop(dev, H, W, layout, cy, cx, h, w):
    """The sub-planes of a device batch [n, 1.5 H W] for the pixel window [cy : cy + h, cx : cx + w] (all even), as a batch of
    its own: contiguous, so 8-byte aligned frames when h and w are multiples of 8."""
    import torch
    y, u, v = split(dev, H, W, layout)
    n = dev.shape[0]
    y = y[:, cy:cy + h, cx:cx + w].reshape(n, -1)
    u = u[:, cy // 2:(cy + h) // 2, cx // 2:(cx + w) // 2]
    v = v[:, cy // 2:(cy + h) // 2, cx // 2:(cx + w) // 2]
    c = torch.cat([u.reshape(n, -1), v.reshape(n, -1)], 1) if layout == "i420" else torch.stack([u, v], -1).reshape(n, -1)
    return torch.cat([y, c], 1).contiguous()


def device_sub(dev, H, W, layout, py, px):
    """sub(py, px) of a device batch and its (rows, cols); None without a unit."""
    r, c = (H - py) // 8, (W - px) // 8
    if r < 1 or c < 1:
        return None, (r, c)
    return device_crop(dev, H, W, layout, py, px, 8 * r, 8 * c), (r, c)


def synthetic_planes(n, H, W, seed, layout):
    return cuda(pr.pack([pr.to_planes(orc.synthetic_frame(H, W, seed + i)) for i in range(n)], layout))


def scores_call(eng, codec, dev, H, W, layout, scores=None, scale=15):
    if codec == "svd":
        return eng.svd_sync_scores_yuv420(dev, H, W, scale=scale, layout=layout, scores=scores)
    return eng.sync_scores_yuv420(dev, H, W, alpha=pr.ALPHA, layout=layout, scores=scores)


def window_call(eng, codec, dev, H, W, L, phase, canvas_cols, base, layout, soft=None, scales=None):
    if codec == "svd":
        return eng.svd_detect_soft_window_yuv420(dev, H, W, L, phase, canvas_cols, base=base, scales=scales, layout=layout, soft=soft)
    return eng.detect_soft_window_yuv420(dev, H, W, L, phase, canvas_cols, base=base, alpha=pr.ALPHA, layout=layout, soft=soft)


def readout(eng, codec, sub, h, w, L, layout, scale=15):
    """The existing planar soft read-out (the reference of every comparison here)."""
    if codec == "svd":
        return eng.svd_detect_soft_yuv420(sub, h, w, L, scale=scale, layout=layout)
    return eng.detect_soft_yuv420(sub, h, w, L, alpha=pr.ALPHA, layout=layout)


def reference_scores(eng, codec, dev, H, W, layout, scale=15):
    ref = np.zeros((dev.shape[0], 64), np.int64)
    for py in range(0, 8, 2):
        for px in range(0, 8, 2):
            sub, (r, c) = device_sub(dev, H, W, layout, py, px)
            if sub is not None:
                ref[:, 8 * py + px] = readout(eng, codec, sub, 8 * r, 8 * c, r * c, layout, scale).abs().sum(dim=1).cpu().numpy()
    return ref


@pytest.fixture(scope="module")
def leaks():
    """The oracle-marked recipe leak of either codec in either layout: CUDA u8 [12, 1.5 * 62 * 84], left unchanged."""
    return {(codec, layout): cuda(pr.pack(pr.oracle_leak(codec), layout)) for codec in pr.CODECS for layout in LAYOUTS}


SHAPES = {"leak-2x62x84": None, "1x100x138": (1, 100, 138), "1x8x8": (1, 8, 8), "1x8x40": (1, 8, 40), "1x40x10": (1, 40, 10),
          "2x10x14": (2, 10, 14)}                             # 10x14: frames 210 bytes apart, frame 1 is only 2-byte aligned


# ---- 1. the dense phase search ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("codec", pr.CODECS)
@pytest.mark.parametrize("shape_id", list(SHAPES))
def test_scores_equal_the_planar_read_out_of_every_even_sub_frame(eng, leaks, shape_id, codec, layout):
    from offmark import resync
    if SHAPES[shape_id] is None:
        dev, (H, W) = leaks[codec, layout][:2].contiguous(), (pr.LEAK_H, pr.LEAK_W)
    else:
        n, H, W = SHAPES[shape_id]
        dev = synthetic_planes(n, H, W, 7300 + H, layout)
    n = dev.shape[0]
    got = scores_call(eng, codec, dev, H, W, layout, scores=garbage(n, 64)).cpu().numpy()
    assert got.shape == (n, 64) and got.dtype == np.int64
    units = np.where(pr.EVEN, resync.units_per_phase(H, W), 0)
    assert (got[:, units == 0] == 0).all() and (got[:, units > 0] > 0).all()      # odd and unit-less entries are exactly 0
    ref = reference_scores(eng, codec, dev, H, W, layout)
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    if SHAPES[shape_id] is None:                                                   # and against the NumPy statement
        for f in range(n):
            want, budget = pr.statement_scores(pr.oracle_leak(codec)[f], codec)
            d = np.abs(got[f] - want)
            print(f"{codec} {layout} frame {f}: worst |device - statement| {d.max()} (budget there {budget[d.argmax()]})")
            assert (d <= budget).all(), (f, d.max(), budget[d.argmax()])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_svd_scores_at_another_scale(eng, leaks, layout):
    dev = leaks["svd", layout][:2].contiguous()
    got = scores_call(eng, "svd", dev, pr.LEAK_H, pr.LEAK_W, layout, scores=garbage(2, 64), scale=3.5).cpu().numpy()
    ref = reference_scores(eng, "svd", dev, pr.LEAK_H, pr.LEAK_W, layout, scale=3.5)
    assert np.array_equal(got, ref) and got[:, pr.EVEN].all()
    assert not np.array_equal(got, scores_call(eng, "svd", dev, pr.LEAK_H, pr.LEAK_W, layout).cpu().numpy())


# ---- 2. the RGB route gives the same even entries ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("codec", pr.CODECS)
def test_scores_equal_the_even_entries_of_the_rgb_search(eng, codec, layout):
    H, W, n = 64, 88, 2
    dev = synthetic_planes(n, H, W, 7400, layout)
    rgb = eng.yuv420_to_rgb(dev, H, W, layout=layout)
    via_rgb = (eng.svd_sync_scores(rgb) if codec == "svd" else eng.sync_scores(rgb, alpha=pr.ALPHA)).cpu().numpy()
    got = scores_call(eng, codec, dev, H, W, layout, scores=garbage(n, 64)).cpu().numpy()
    assert np.array_equal(got[:, pr.EVEN], via_rgb[:, pr.EVEN]) and got[:, pr.EVEN].all()
    assert (got[:, ~pr.EVEN] == 0).all() and via_rgb[:, ~pr.EVEN].all()


# ---- 3. the window read-out --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("codec", pr.CODECS)
@pytest.mark.parametrize("base", [0, 29])
@pytest.mark.parametrize("phase", [(6, 4), (0, 0), (6, 6)])
def test_window_equals_the_sub_frame_read_out_regrouped(eng, leaks, phase, base, codec, layout):
    dev, H, W = leaks[codec, layout], pr.LEAK_H, pr.LEAK_W
    n = dev.shape[0]
    sub, (r, c) = device_sub(dev, H, W, layout, *phase)
    per_unit = readout(eng, codec, sub, 8 * r, 8 * c, r * c, layout).cpu().numpy()
    assert (per_unit != 0).mean() > 0.9
    for L in (8, 5, 77, 3000):                                                 # 3000: past the LDS histogram
        got = window_call(eng, codec, dev, H, W, L, phase, 13, base, layout, soft=garbage(n, L)).cpu().numpy()
        ref = np.stack([pr.canvas_regroup(per_unit[f], r, c, 13, base, L) for f in range(n)])
        assert got.shape == (n, L) and got.dtype == np.int64 and np.array_equal(got, ref), (L, np.argwhere(got != ref)[:5])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("codec", pr.CODECS)
def test_window_at_the_origin_is_the_planar_soft_read_out(eng, codec, layout):
    import torch
    H, W, n = 64, 96, 3
    dev = synthetic_planes(n, H, W, 7500, layout)
    for L in (8, 5, 96, 3000):
        got = window_call(eng, codec, dev, H, W, L, (0, 0), W // 8, 0, layout, soft=garbage(n, L))
        assert torch.equal(got, readout(eng, codec, dev, H, W, L, layout)) and got.any()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_svd_window_with_channel_1_unmarked_gives_zeros(eng, leaks, layout):
    dev = leaks["svd", layout]
    got = window_call(eng, "svd", dev, pr.LEAK_H, pr.LEAK_W, 8, pr.PHASE, 13, 0, layout, soft=garbage(dev.shape[0], 8), scales=(10, 0, 20))
    assert not got.any()


# ---- 4. the launch-chunk edge ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", pr.CODECS)
def test_rows_past_the_launch_chunk_equal_the_call_on_the_tail(eng, codec):
    """65537 frames: the library launches at most 65535 at a time, so the last two go through a launch of their own.  The DCT
    calls go through the library with one workspace for all frames and chunk_frames = 0, so that clamp is the library's."""
    import torch
    from offmark import _hip
    n, H, W, L, layout = 65537, 8, 10, 8, "i420"
    g = torch.Generator(device="cuda").manual_seed(11)
    dev = torch.randint(0, 256, (n, H * W * 3 // 2), dtype=torch.uint8, device="cuda", generator=g)
    tail = dev[65535:].contiguous()
    stream = _hip.current_stream()

    def both(frames):
        k = frames.shape[0]
        scores, soft = garbage(k, 64), garbage(k, L)
        if codec == "svd":
            eng.svd_sync_scores_yuv420(frames, H, W, layout=layout, scores=scores)
            eng.svd_detect_soft_window_yuv420(frames, H, W, L, (0, 2), 3, base=5, layout=layout, soft=soft)
        else:
            ws = torch.empty(eng.lib.ofmk_sync_workspace_bytes_yuv420(min(k, 65535), H, W), dtype=torch.uint8, device="cuda")
            _hip.check(eng.lib.ofmk_sync_scores_yuv420(frames.data_ptr(), 0, k, H, W, 20.0, scores.data_ptr(), 0, ws.data_ptr(), ws.numel(),
                                                       stream, None))
            wws = torch.empty(eng.lib.ofmk_workspace_bytes(min(k, 65535), 8, 8), dtype=torch.uint8, device="cuda")
            _hip.check(eng.lib.ofmk_detect_soft_window_yuv420(frames.data_ptr(), 0, k, H, W, 0, 2, 3, 5, L, 20.0, soft.data_ptr(), 0,
                                                              wws.data_ptr(), wws.numel(), stream, None))
            torch.cuda.synchronize()                          # the workspaces go out of scope here
        return scores, soft

    (s_all, w_all), (s_tail, w_tail) = both(dev), both(tail)
    assert torch.equal(s_all[65535:], s_tail) and torch.equal(w_all[65535:], w_tail)
    assert s_tail[:, [0, 2]].any() and w_tail.any() and s_all[:65535, [0, 2]].any() and not s_all[:, 1].any()
    head = both(dev[:3].contiguous())
    assert torch.equal(s_all[:3], head[0]) and torch.equal(w_all[:3], head[1])


def test_small_planes_in_chunks_of_two_equal_the_librarys_own_chunking(eng):
    """The DCT calls on 5 random I420 frames of 22x36 -- no multiple of 8, a nonzero phase, a partial last chunk, frame offsets
    into the shared records -- with chunk_frames = 2 and with chunk_frames = 0 (one chunk: the workspace holds all five), each
    call on a workspace sized for it."""
    import torch
    from offmark import _hip
    n, H, W, L = 5, 22, 36, 8
    g = torch.Generator(device="cuda").manual_seed(22)
    dev = torch.randint(0, 256, (n, H * W * 3 // 2), dtype=torch.uint8, device="cuda", generator=g)
    stream = _hip.current_stream()
    rows, cols = (H - 2) // 8, (W - 6) // 8

    def both(cf):
        scores, soft = garbage(n, 64), garbage(n, L)
        ws = torch.empty(eng.lib.ofmk_sync_workspace_bytes_yuv420(cf or n, H, W), dtype=torch.uint8, device="cuda")
        _hip.check(eng.lib.ofmk_sync_scores_yuv420(dev.data_ptr(), 0, n, H, W, 20.0, scores.data_ptr(), cf, ws.data_ptr(), ws.numel(), stream,
                                                   None))
        wws = torch.empty(eng.lib.ofmk_workspace_bytes(cf or n, 8 * rows, 8 * cols), dtype=torch.uint8, device="cuda")
        _hip.check(eng.lib.ofmk_detect_soft_window_yuv420(dev.data_ptr(), 0, n, H, W, 2, 6, 7, 3, L, 20.0, soft.data_ptr(), cf, wws.data_ptr(),
                                                          wws.numel(), stream, None))
        torch.cuda.synchronize()                              # the workspaces go out of scope here
        return scores, soft

    (s2, w2), (s0, w0) = both(2), both(0)
    assert torch.equal(s2, s0) and torch.equal(w2, w0)
    assert s0.any() and w0.any()


# ---- 5. end to end on the device ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("codec", pr.CODECS)
def test_a_cropped_planar_leak_is_read_end_to_end(eng, codec, layout):
    from offmark import resync
    from offmark.dist.vote import soft_vote
    from offmark.degenerator.de_shuffler import DeShuffler
    from offmark.extract.dct_decoder import DctDecoder
    from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder
    from offmark.generator.shuffler import Shuffler
    pay, seg = pr.recipe_payloads(), pr.recipe_segments()
    wm = np.stack([Shuffler(key=pr.KEY).generate_wm(p, (pr.H * pr.W // 64,)) for p in pay]).astype(np.uint8)
    src = cuda(pr.pack([pr.to_planes(f) for f in pr.recipe_sources()], layout))
    rows = cuda(seg.astype(np.int32))
    if codec == "svd":
        marked = eng.svd_embed_yuv420(src, pr.H, pr.W, wm, scale=15, wm_row=rows, layout=layout)
        decoder = DwtDctSvdDecoder()
    else:
        marked = eng.embed_yuv420(src, pr.H, pr.W, wm, alpha=pr.ALPHA, wm_row=rows, layout=layout)
        decoder = DctDecoder(alpha=pr.ALPHA)
    leak = device_crop(marked, pr.H, pr.W, layout, pr.CROP[0], pr.CROP[1], pr.LEAK_H, pr.LEAK_W)
    assert tuple(leak.shape) == (12, 62 * 84 * 3 // 2)
    got = resync.read_cropped_leak_yuv420(decoder, leak, pr.LEAK_H, pr.LEAK_W, seg, pr.W, pr.recipe_candidates(), key=pr.KEY, L=pr.L8,
                                          layout=layout)
    print(f"{codec} {layout}: phase {got['phase']} contrast {got['contrast']:.3f} base {got['base']} picks {list(got['picks'])} "
          f"score {got['score']} runner-up {got['runner_up_score']}")
    assert got["phase"] == pr.PHASE and got["base"] == pr.BASE and list(got["picks"]) == list(pr.CHOSEN) and not got["ambiguous"]
    assert got["contrast"] > {"svd": 1.2, "dct": 1.06}[codec]
    # what the feature buys: the plain planar soft read-out of the same leak, trimmed to 56x80 at phase (0, 0), read by sign
    plain = readout(eng, codec, device_crop(leak, pr.LEAK_H, pr.LEAK_W, layout, 0, 0, 56, 80), 56, 80, pr.L8, layout).cpu().numpy()
    by_sign = soft_vote(plain, DeShuffler(key=pr.KEY).set_shape((pr.L8,)).payload_idx, seg)
    right = sum(int(np.array_equal(by_sign[s], pay[s])) for s in range(pr.S))
    print(f"plain read-out at phase (0, 0): {right}/3 segments by sign")
    assert right < 3


# ---- 6. graph capture ----------------------------------------------------------------------------------------------------------
def test_all_four_calls_are_graph_capturable(eng, leaks):
    """No allocation and no synchronisation inside the calls: they capture into a HIP graph and replay with identical results."""
    import torch
    layout, H, W = "nv12", pr.LEAK_H, pr.LEAK_W
    svd, dct = leaks["svd", layout], leaks["dct", layout]
    n = svd.shape[0]

    def run(out):
        scores_call(eng, "svd", svd, H, W, layout, scores=out[0])
        window_call(eng, "svd", svd, H, W, 8, pr.PHASE, 13, 3, layout, soft=out[1])
        scores_call(eng, "dct", dct, H, W, layout, scores=out[2])
        window_call(eng, "dct", dct, H, W, 8, pr.PHASE, 13, 3, layout, soft=out[3])

    ref = [garbage(n, 64), garbage(n, 8), garbage(n, 64), garbage(n, 8)]
    run(ref)
    torch.cuda.synchronize()
    out = [garbage(n, 64), garbage(n, 8), garbage(n, 64), garbage(n, 8)]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        run(out)                                             # warm-up on the capture stream
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            run(out)
    for o in out:
        o.fill_(7)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) and a.any() for a, b in zip(out, ref))
    del graph
    import gc
    gc.collect()
    torch.cuda.synchronize()


# ---- 7. workspace ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_dct_calls_with_a_one_frame_workspace(eng, leaks, layout):
    import torch
    from offmark import _hip
    dev, H, W, lay = leaks["dct", layout][:5].contiguous(), pr.LEAK_H, pr.LEAK_W, eng._layout(layout)
    n, stream = dev.shape[0], _hip.current_stream()
    need = eng.lib.ofmk_sync_workspace_bytes_yuv420(1, H, W)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    scores = garbage(n, 64)
    rc = eng.lib.ofmk_sync_scores_yuv420(dev.data_ptr(), lay, n, H, W, 20.0, scores.data_ptr(), 0, ws.data_ptr(), need - 1, stream, None)
    assert rc == -2 and eng.lib.ofmk_last_error().decode() != ""
    _hip.check(eng.lib.ofmk_sync_scores_yuv420(dev.data_ptr(), lay, n, H, W, 20.0, scores.data_ptr(), 0, ws.data_ptr(), need, stream, None))
    assert torch.equal(scores, eng.sync_scores_yuv420(dev, H, W, layout=layout)) and scores[:, 0].all()
    rows, cols = (H - pr.PHASE[0]) // 8, (W - pr.PHASE[1]) // 8
    need = eng.lib.ofmk_workspace_bytes(1, 8 * rows, 8 * cols)
    wws = torch.empty(need, dtype=torch.uint8, device="cuda")
    soft = garbage(n, 8)
    args = (dev.data_ptr(), lay, n, H, W, pr.PHASE[0], pr.PHASE[1], 13, 29, 8, 20.0, soft.data_ptr(), 0, wws.data_ptr())
    rc = eng.lib.ofmk_detect_soft_window_yuv420(*args, need - 1, stream, None)
    assert rc == -2 and eng.lib.ofmk_last_error().decode() != ""
    _hip.check(eng.lib.ofmk_detect_soft_window_yuv420(*args, need, stream, None))
    assert torch.equal(soft, eng.detect_soft_window_yuv420(dev, H, W, 8, pr.PHASE, 13, base=29, layout=layout)) and soft.any()
    torch.cuda.synchronize()
