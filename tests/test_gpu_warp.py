"""GPU: reading rescaled leaks (engine.warp / svd_warp_scores / svd_detect_soft_warp, the decoders' decode_soft_warp_u8,
offmark.resync.read_rescaled_leak; build extensions, not reference semantics).

The warp is defined in integers, so the device equals the NumPy statement (tests/_warp.py) byte for byte.  The fused calls are held
against the chain they replace -- warp of the counting rectangle, then the existing read-outs -- integer for integer, nothing
masked out.  End to end the recipe is marked on the device and attacked on the host (tests/_warp.py: float64 bilinear)."""
import numpy as np
import pytest

import offmark_oracle as orc
import _resync as rs
import _warp as wp

pytestmark = pytest.mark.gpu

ONE = 65536
CANVAS = (wp.H, wp.W)                        # 72 x 104
SHIFT = (ONE, -(11 << 16), ONE, -(21 << 16))                 # the cropped recipe as a warp: negative by / bx
DOWN = (49152, -8192, 49152, -8192)                          # a 0.75x leak (54 x 78 of the canvas' 72 x 104), half-pixel centres
UP = (98304, 16384, 98304, 16384)                            # a 1.5x leak
NO_UNIT = (ONE, 1 << 40, ONE, 0)
ONE_UNIT = (ONE, -(58 << 16), ONE, -(90 << 16))              # of a 61 x 83 leak only canvas unit (8, 12) is wholly inside


@pytest.fixture(scope="module")
def eng():
    import torch
    from offmark.engine import DctEngine
    torch.cuda.set_device(0)
    return DctEngine()


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the shared references are read-only


def garbage(shape, dtype=None):
    """The output buffer a call gets holds anything: the library writes or clears all of it."""
    import torch
    if dtype is torch.uint8:
        return torch.full(shape, 0x5A, dtype=torch.uint8, device="cuda")
    return torch.full(shape, 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")


@pytest.fixture(scope="module")
def leak61():
    """5 frames of the cropped recipe, 61 x 83: sizes that are no multiple of anything."""
    return np.array(rs.oracle_leak()[:5])


@pytest.fixture(scope="module")
def zoom():
    """5 frames of the oracle-marked recipe cropped 5:67 / 7:99 and resized back to 72 x 104."""
    return np.array(wp.leak("svd")[:5])


def chain_rect(eng, dev, canvas, g):
    """The warp of the counting rectangle of geometry g, and the rectangle; (None, zeros) when no unit counts."""
    r = eng.warp_units(tuple(dev.shape[1:3]), canvas, g)
    if r[1] == r[0]:
        return None, r
    return eng.warp(dev, g, (8 * (r[1] - r[0]), 8 * (r[3] - r[2])), origin=(8 * r[0], 8 * r[2])), r


# ---- 1. the warp against the statement ------------------------------------------------------------------------------------------
WARPS = {"identity": ("leak61", wp.IDENTITY, (61, 83), (0, 0)), "shift": ("leak61", SHIFT, (72, 104), (0, 0)),
         "zoom-back": ("zoom", None, (72, 104), (0, 0)), "zoom-back-odd-size": ("zoom", None, (70, 99), (0, 0)),
         "0.75x": ("leak61", DOWN, (85, 113), (0, 0)), "1.5x": ("leak61", UP, (43, 59), (0, 0)),
         "window": ("zoom", None, (37, 45), (8, 16)), "window-past-the-leak": ("leak61", SHIFT, (29, 50), (50, 70))}


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("case", list(WARPS))
def test_warp_equals_the_statement(eng, request, case, n):
    import torch
    which, g, out_hw, origin = WARPS[case]
    frames = request.getfixturevalue(which)[:n]
    g = wp.true_geometry() if g is None else g
    got = eng.warp(cuda(frames), g, out_hw, origin=origin, out=garbage((n, *out_hw, 3), torch.uint8)).cpu().numpy()
    ref = np.stack([wp.warp(f, g, out_hw, origin)[0] for f in frames])
    assert got.shape == ref.shape and got.dtype == np.uint8 and np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    if case == "identity":
        assert np.array_equal(got, frames)                                    # the frame itself
    else:
        assert ref.any()


# ---- 2. the fused scores against the chain --------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [15, 3.5])
def test_scores_equal_the_chain(eng, leak61, scale):
    dev = cuda(leak61)
    n = dev.shape[0]
    cands = np.array([wp.IDENTITY, SHIFT, DOWN, UP, NO_UNIT, ONE_UNIT, (ONE, -(3 << 16) - 77, ONE, -(2 << 16) - 40000),
                      wp.true_geometry((61, 83))], np.int64)
    got = eng.svd_warp_scores(dev, CANVAS, cands, scale=scale, scores=garbage((n, len(cands)))).cpu().numpy()
    assert got.shape == (n, len(cands)) and got.dtype == np.int64
    ref = np.zeros_like(got)
    units = []
    for k, g in enumerate(cands):
        rect, r = chain_rect(eng, dev, CANVAS, g)
        units.append((r[1] - r[0]) * (r[3] - r[2]))
        if rect is not None:
            ref[:, k] = eng.svd_sync_scores(rect, scale=scale)[:, 0].cpu().numpy()
    assert units[4] == 0 and units[5] == 1 and min(units[:4]) > 1
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    assert not got[:, 4].any() and (got[:, np.array(units) > 0] > 0).all()     # a candidate without a counting unit scores 0


def test_scores_on_the_zoomed_leak_and_at_the_identity(eng, zoom):
    import torch
    dev = cuda(zoom)
    n = dev.shape[0]
    cands = wp.candidate_geometries()
    got = eng.svd_warp_scores(dev, CANVAS, torch.from_numpy(cands).cuda()).cpu().numpy()     # a device tensor is taken as it is
    for k in (0, 1, 17, 30, 49):
        rect, _ = chain_rect(eng, dev, CANVAS, cands[k])
        assert np.array_equal(got[:, k], eng.svd_sync_scores(rect)[:, 0].cpu().numpy()), k
    ident = eng.svd_warp_scores(dev, CANVAS, np.array([wp.IDENTITY]))          # an uncropped 72 x 104 frame: every unit counts
    assert torch.equal(ident[:, 0], eng.svd_sync_scores(dev)[:, 0]) and ident.all()


def test_scores_of_candidates_past_a_launch_chunk(eng):
    """More candidates than one launch takes (65535 sit in gridDim.y): the second launch's candidates and columns start where the
    first one's end.  An 8 x 8 leak on an 8 x 8 canvas: one unit per candidate, sub-pixel shifts that stay inside."""
    import torch
    K, edge, n = 65537, 65535, 2
    g = torch.Generator(device="cuda")
    g.manual_seed(12)
    frames = torch.randint(0, 256, (n, 8, 8, 3), dtype=torch.uint8, device="cuda", generator=g)
    k = np.arange(K, dtype=np.int64)
    cands = torch.from_numpy(np.stack([np.full(K, ONE), 256 * (k % 251), np.full(K, ONE), 256 * (k % 241)], axis=1)).cuda()
    full = eng.svd_warp_scores(frames, (8, 8), cands, scores=garbage((n, K)))
    assert torch.equal(full[:, edge - 3:], eng.svd_warp_scores(frames, (8, 8), cands[edge - 3:].contiguous()))
    assert torch.equal(full[:, :5], eng.svd_warp_scores(frames, (8, 8), cands[:5].contiguous()))
    assert (full > 0).float().mean() > 0.9
    for kk in (edge - 1, edge, K - 1):
        rect = eng.warp(frames, cands[kk].cpu().numpy(), (8, 8))
        assert torch.equal(full[:, kk], eng.svd_sync_scores(rect)[:, 0]), kk


# ---- 3. the fused read-out against the chain --------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,g", [("zoom", None), ("leak61", SHIFT), ("leak61", DOWN), ("leak61", UP), ("leak61", ONE_UNIT)])
def test_read_out_equals_the_chain(eng, request, which, g):
    dev = cuda(request.getfixturevalue(which))
    n = dev.shape[0]
    g = wp.true_geometry() if g is None else g
    rect, (i0, i1, j0, j1) = chain_rect(eng, dev, CANVAS, g)
    cw = wp.W // 8
    for L in (8, 5, 3000):                                                     # 3000: past the LDS histogram
        got = eng.svd_detect_soft_warp(dev, CANVAS, g, L, soft=garbage((n, L)))
        ref = eng.svd_detect_soft_window(rect, L, (0, 0), cw, base=i0 * cw + j0)
        assert got.shape == (n, L) and got.dtype == ref.dtype and np.array_equal(got.cpu().numpy(), ref.cpu().numpy()), L
        assert got.any()
    z = eng.svd_detect_soft_warp(dev, CANVAS, NO_UNIT, 8, soft=garbage((n, 8)))
    assert not z.any()                                                         # no counting unit: zeros, not an error
    z = eng.svd_detect_soft_warp(dev, CANVAS, g, 8, scales=(10, 0, 20), soft=garbage((n, 8)))
    assert not z.any()                                                         # channel 1 unmarked: zeros, as the soft read-out


def test_read_out_at_the_identity_is_the_soft_read_out(eng):
    import torch
    dev = cuda(np.stack([orc.synthetic_frame(wp.H, wp.W, 7200 + i) for i in range(3)]))
    for L in (8, 5):
        got = eng.svd_detect_soft_warp(dev, CANVAS, wp.IDENTITY, L)
        assert torch.equal(got, eng.svd_detect_soft(dev, L)) and got.any()


def test_the_dct_decoder_reads_through_the_chain(eng, zoom):
    import torch
    from offmark.extract.dct_decoder import DctDecoder
    dev = cuda(zoom)
    g = wp.true_geometry()
    dec = DctDecoder(alpha=20)
    rect, (i0, i1, j0, j1) = chain_rect(dec.engine, dev, CANVAS, g)
    cw = wp.W // 8
    for L in (8, 5):
        got = dec.decode_soft_warp_u8(dev, CANVAS, g, L)
        assert torch.equal(got, dec.engine.detect_soft_window(rect, L, (0, 0), cw, base=i0 * cw + j0, alpha=20)) and got.any()
    assert not dec.decode_soft_warp_u8(dev, CANVAS, NO_UNIT, 8).any()


# ---- 4. end to end on the device ------------------------------------------------------------------------------------------------
def device_marked(eng, codec):
    """The recipe marked ON THE DEVICE (one watermark row per segment), back on the host: u8 [12, 72, 104, 3]."""
    from offmark.generator.shuffler import Shuffler
    pay, seg = rs.recipe_payloads(), rs.recipe_segments()
    wm = np.stack([Shuffler(key=wp.KEY).generate_wm(p, (wp.H * wp.W // 64,)) for p in pay]).astype(np.uint8)
    src, rows = cuda(rs.recipe_sources()), cuda(seg.astype(np.int32))
    marked = eng.svd_embed(src, wm, wm_row=rows) if codec == "svd" else eng.embed(src, wm, alpha=20, wm_row=rows)
    return marked.cpu().numpy()


def decoder_of(codec):
    from offmark.extract.dct_decoder import DctDecoder
    from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder
    return DwtDctSvdDecoder() if codec == "svd" else DctDecoder(alpha=20)


def test_a_zoomed_back_leak_is_found_and_read(eng):
    from offmark import resync
    leak = cuda(wp.attack(device_marked(eng, "svd"), wp.CROP, wp.ZOOM_HW))
    cands = wp.candidate_geometries()
    got = resync.read_rescaled_leak(decoder_of("svd"), leak, rs.recipe_segments(), CANVAS, rs.recipe_candidates(), cands, key=wp.KEY,
                                    L=wp.L8, search_frames=wp.SEARCH_FRAMES)
    n = got["normalised"]
    print(f"index {got['index']} true {n[0]:.4f} best other {np.delete(n, 0).max():.4f} contrast {got['contrast']:.4f} picks {[int(p) for p in got['picks']]}")
    assert got["index"] == 0 and got["geometry"] == tuple(cands[0])
    assert list(got["picks"]) == list(wp.CHOSEN) and not got["ambiguous"] and got["base"] == 0


@pytest.mark.parametrize("leak_hw", [wp.ZOOM_HW, wp.DOWN_HW])
@pytest.mark.parametrize("codec", ["svd", "dct"])
def test_both_codecs_read_at_the_known_geometry(eng, codec, leak_hw):
    from offmark import resync
    leak = cuda(wp.attack(device_marked(eng, codec), wp.CROP, leak_hw))
    assert tuple(leak.shape) == (12, *leak_hw, 3)
    got = resync.read_rescaled_leak(decoder_of(codec), leak, rs.recipe_segments(), CANVAS, rs.recipe_candidates(),
                                    [wp.true_geometry(leak_hw)], key=wp.KEY, L=wp.L8)
    print(f"{codec} {leak_hw}: picks {[int(p) for p in got['picks']]} score {got['score']}")
    assert list(got["picks"]) == list(wp.CHOSEN) and not got["ambiguous"] and got["contrast"] is None


# ---- 5. graph capture -----------------------------------------------------------------------------------------------------------
def test_all_three_calls_are_graph_capturable(eng, zoom):
    """No allocation and no synchronisation inside the calls: they capture into a HIP graph and replay with identical results."""
    import torch
    dev = cuda(zoom)
    n = dev.shape[0]
    g = wp.true_geometry()
    cands = torch.from_numpy(wp.candidate_geometries()[:7]).cuda()
    ref_warp = eng.warp(dev, g, (70, 99), origin=(1, 2))
    ref_scores = eng.svd_warp_scores(dev, CANVAS, cands)
    ref_soft = eng.svd_detect_soft_warp(dev, CANVAS, g, 8)
    torch.cuda.synchronize()
    out, scores, soft = garbage((n, 70, 99, 3), torch.uint8), garbage((n, 7)), garbage((n, 8))
    stream = torch.cuda.Stream()

    def calls():
        eng.warp(dev, g, (70, 99), origin=(1, 2), out=out)
        eng.svd_warp_scores(dev, CANVAS, cands, scores=scores)
        eng.svd_detect_soft_warp(dev, CANVAS, g, 8, soft=soft)

    with torch.cuda.stream(stream):
        calls()                                              # warm-up on the capture stream
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            calls()
    out.fill_(7)
    scores.fill_(7)
    soft.fill_(7)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref_warp) and torch.equal(scores, ref_scores) and torch.equal(soft, ref_soft)
    del graph
    import gc
    gc.collect()
    torch.cuda.synchronize()
