"""GPU: block-grid resync of cropped frames with the DCT codec (engine.sync_scores / detect_soft_window, offmark.resync; build
extensions, not reference semantics).

Device against device is exact, integer for integer, nothing masked out, output buffers pre-filled with garbage: the dense phase
search against 64 stand-alone soft read-outs of the 64 shifted contiguous crops -- each with its own crop's frame mean -- and the
window read-out against the per-block read-out of the crop regrouped on the host.  The statement over the oracle is
tests/test_dct_resync_statement.py's."""
import numpy as np
import pytest

import offmark_oracle as orc
import _dct_resync as dr

pytestmark = pytest.mark.gpu


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


def device_crop(dev, py, px):
    """The contiguous crop holding the full blocks of phase (py, px) of a device batch, and its (rows, cols); None without a block."""
    H, W = dev.shape[1:3]
    r, c = (H - py) // 8, (W - px) // 8
    if r < 1 or c < 1:
        return None, (r, c)
    return dev[:, py:py + 8 * r, px:px + 8 * c].contiguous(), (r, c)


@pytest.fixture(scope="module")
def leak(eng):
    """The recipe marked ON THE DEVICE (one watermark row per segment) and cropped: CUDA u8 [12, 61, 83, 3], left unchanged."""
    from offmark.generator.shuffler import Shuffler
    pay, seg = dr.recipe_payloads(), dr.recipe_segments()
    wm = np.stack([Shuffler(key=dr.KEY).generate_wm(p, (dr.H * dr.W // 64,)) for p in pay]).astype(np.uint8)
    marked = eng.embed(cuda(dr.recipe_sources()), wm, alpha=dr.ALPHA, wm_row=cuda(seg.astype(np.int32)))
    out = marked[:, dr.CROP[0]:, dr.CROP[1]:].contiguous()
    assert tuple(out.shape) == (12, 61, 83, 3)
    return out


SHAPES = {"leak-4x61x83": None, "1x100x139": (1, 100, 139), "1x8x8": (1, 8, 8), "1x8x40": (1, 8, 40), "1x40x9": (1, 40, 9)}


def crop_mean(frame, py, px):
    """mean(A00 / 8) of the phase's crop, i.e. the mean of Y over it, as the luminance mask's frame mean (before its clamp at 90)."""
    crop, _ = dr.window(frame, py, px)
    f = crop.astype(np.float64)
    return float((0.114 * f[..., 0] + 0.587 * f[..., 1] + 0.299 * f[..., 2]).mean())


# ---- 1. the dense phase search ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [20, 10])
@pytest.mark.parametrize("shape_id", list(SHAPES))
def test_scores_equal_the_soft_read_out_of_every_shifted_crop(eng, leak, shape_id, alpha):
    if SHAPES[shape_id] is None:
        dev = leak[:4].contiguous()
        host = dev.cpu().numpy()
        # the four brightness offsets of synthetic_frame: frame means on both sides of the luminance mask's clamp at 90, and a
        # mean that moves with the phase (a single frame-wide mean would be wrong for 63 of the 64 crops)
        means = np.array([[crop_mean(f, py, px) for py in range(8) for px in range(8)] for f in host])
        print("crop means per frame, min..max over the 64 phases:", [(round(m.min(), 2), round(m.max(), 2)) for m in means])
        assert (means.max(axis=1) > 95).any() and (means.max(axis=1) < 85).any()
        bright = means[means.max(axis=1) > 95]
        assert (bright.min(axis=1) > 90).any() and (bright.max(axis=1) - bright.min(axis=1) > 0.1).all()
    else:
        n, H, W = SHAPES[shape_id]
        dev = cuda(np.stack([orc.synthetic_frame(H, W, 7000 + H + i) for i in range(n)]))
    n, H, W = dev.shape[:3]
    got = eng.sync_scores(dev, alpha=alpha, scores=garbage(n, 64)).cpu().numpy()
    assert got.shape == (n, 64) and got.dtype == np.int64
    ref = np.zeros((n, 64), np.int64)
    for py in range(8):
        for px in range(8):
            crop, (r, c) = device_crop(dev, py, px)
            if crop is not None:
                ref[:, 8 * py + px] = eng.detect_soft(crop, r * c, alpha=alpha).abs().sum(dim=1).cpu().numpy()
    from offmark import resync
    units = resync.units_per_phase(H, W)
    assert (got[:, units == 0] == 0).all() and (got[:, units > 0] > 0).all()   # a phase without units scores exactly 0
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]


# ---- 2. chunking, through the library -------------------------------------------------------------------------------------
def test_chunks_of_two_frames_equal_one_chunk(eng, leak):
    import torch
    from offmark import _hip
    dev = leak[:5].contiguous()
    n, H, W = dev.shape[:3]
    stream = _hip.current_stream()
    ws = eng.sync_workspace(H, W, n)

    def scores(cf):
        out = garbage(n, 64)
        _hip.check(eng.lib.ofmk_sync_scores_rgb8(dev.data_ptr(), n, H, W, 20.0, out.data_ptr(), cf, ws.data_ptr(), ws.numel(), stream, None))
        return out

    assert torch.equal(scores(2), scores(n)) and scores(2).any()
    rows, cols = (H - 5) // 8, (W - 3) // 8
    wws = torch.empty(eng.lib.ofmk_workspace_bytes(n, 8 * rows, 8 * cols), dtype=torch.uint8, device="cuda")

    def window(cf):
        out = garbage(n, 8)
        _hip.check(eng.lib.ofmk_detect_soft_window_rgb8(dev.data_ptr(), n, H, W, 5, 3, 13, 29, 8, 20.0, out.data_ptr(), cf, wws.data_ptr(),
                                                        wws.numel(), stream, None))
        return out

    assert torch.equal(window(2), window(n)) and window(2).any()
    assert torch.equal(window(2), eng.detect_soft_window(dev, 8, (5, 3), 13, base=29))
    assert torch.equal(scores(2), eng.sync_scores(dev))


def test_small_frames_in_chunks_of_two_equal_the_librarys_own_chunking(eng):
    """5 random frames of 23x37 -- no multiple of 8, a nonzero phase, a partial last chunk, frame offsets into the shared records --
    with chunk_frames = 2 and with chunk_frames = 0 (one chunk: the workspace holds all five), each call on a workspace sized
    for it."""
    import torch
    from offmark import _hip
    n, H, W, L = 5, 23, 37, 8
    g = torch.Generator(device="cuda").manual_seed(23)
    dev = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    stream = _hip.current_stream()
    rows, cols = (H - 5) // 8, (W - 3) // 8

    def both(cf):
        scores, soft = garbage(n, 64), garbage(n, L)
        ws = torch.empty(eng.lib.ofmk_sync_workspace_bytes(cf or n, H, W), dtype=torch.uint8, device="cuda")
        _hip.check(eng.lib.ofmk_sync_scores_rgb8(dev.data_ptr(), n, H, W, 20.0, scores.data_ptr(), cf, ws.data_ptr(), ws.numel(), stream, None))
        wws = torch.empty(eng.lib.ofmk_workspace_bytes(cf or n, 8 * rows, 8 * cols), dtype=torch.uint8, device="cuda")
        _hip.check(eng.lib.ofmk_detect_soft_window_rgb8(dev.data_ptr(), n, H, W, 5, 3, 7, 3, L, 20.0, soft.data_ptr(), cf, wws.data_ptr(),
                                                        wws.numel(), stream, None))
        torch.cuda.synchronize()                              # the workspaces go out of scope here
        return scores, soft

    (s2, w2), (s0, w0) = both(2), both(0)
    assert torch.equal(s2, s0) and torch.equal(w2, w0)
    assert s0.any() and w0.any()


# ---- 3. the window read-out --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 29])
@pytest.mark.parametrize("phase", [(5, 3), (0, 0), (7, 7)])
def test_window_equals_the_crop_read_out_regrouped(eng, leak, phase, base):
    n = leak.shape[0]
    crop, (r, c) = device_crop(leak, *phase)
    per_unit = eng.detect_soft(crop, r * c).cpu().numpy()
    assert (per_unit != 0).mean() > 0.9
    for L in (8, 5, 77, 3000):                                                 # 3000: past the LDS histogram
        got = eng.detect_soft_window(leak, L, phase, 13, base=base, soft=garbage(n, L)).cpu().numpy()
        ref = np.stack([dr.canvas_regroup(per_unit[f], r, c, 13, base, L) for f in range(n)])
        assert got.shape == (n, L) and got.dtype == np.int64 and np.array_equal(got, ref), (L, np.argwhere(got != ref)[:5])


# ---- 4. the window at the origin ------------------------------------------------------------------------------------------------
def test_window_at_the_origin_is_the_soft_read_out(eng):
    import torch
    H, W, n = 64, 96, 3
    dev = cuda(np.stack([orc.synthetic_frame(H, W, 7100 + i) for i in range(n)]))
    for L in (8, 5, 96, 3000):
        got = eng.detect_soft_window(dev, L, (0, 0), W // 8, soft=garbage(n, L))
        assert torch.equal(got, eng.detect_soft(dev, L)) and got.any()


# ---- 5. end to end on the device ----------------------------------------------------------------------------------------------
def test_a_cropped_leak_is_read_end_to_end(eng, leak):
    from offmark import resync
    from offmark.dist.vote import soft_vote
    from offmark.degenerator.de_shuffler import DeShuffler
    from offmark.extract.dct_decoder import DctDecoder
    pay, seg = dr.recipe_payloads(), dr.recipe_segments()
    got = resync.read_cropped_leak(DctDecoder(), leak, seg, dr.W, dr.recipe_candidates(), key=dr.KEY, L=dr.L8)
    print(f"phase {got['phase']} contrast {got['contrast']:.3f} base {got['base']} picks {list(got['picks'])} "
          f"score {got['score']} runner-up {got['runner_up_score']}")
    assert got["phase"] == dr.PHASE and got["base"] == dr.BASE and list(got["picks"]) == list(dr.CHOSEN) and not got["ambiguous"]
    assert got["contrast"] > 1.1
    # what the feature buys: the plain soft read-out of the same leak, cut to a multiple of 8 at phase (0, 0), read by sign
    plain = eng.detect_soft(leak[:, :56, :80].contiguous(), dr.L8).cpu().numpy()
    by_sign = soft_vote(plain, DeShuffler(key=dr.KEY).set_shape((dr.L8,)).payload_idx, seg)
    right = sum(int(np.array_equal(by_sign[s], pay[s])) for s in range(dr.S))
    print(f"plain read-out at phase (0, 0): {right}/3 segments by sign")
    assert right < 3


# ---- 6. graph capture ----------------------------------------------------------------------------------------------------------
def test_both_calls_are_graph_capturable(eng, leak):
    """No allocation and no synchronisation inside the calls: they capture into a HIP graph and replay with identical results."""
    import torch
    n = leak.shape[0]
    ref_scores = eng.sync_scores(leak)
    ref_soft = eng.detect_soft_window(leak, 8, dr.PHASE, 13, base=3)
    torch.cuda.synchronize()
    scores, soft = garbage(n, 64), garbage(n, 8)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng.sync_scores(leak, scores=scores)                 # warm-up on the capture stream
        eng.detect_soft_window(leak, 8, dr.PHASE, 13, base=3, soft=soft)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            eng.sync_scores(leak, scores=scores)
            eng.detect_soft_window(leak, 8, dr.PHASE, 13, base=3, soft=soft)
    scores.fill_(7)
    soft.fill_(7)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(scores, ref_scores) and torch.equal(soft, ref_soft)
    del graph
    import gc
    gc.collect()
    torch.cuda.synchronize()
