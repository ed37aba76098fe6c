"""GPU: block-grid resync of cropped DwtDctSvd frames (engine.svd_sync_scores / svd_detect_soft_window, offmark.resync; build
extensions, not reference semantics).

Everything that compares the device with itself is exact, integer for integer, nothing masked out: the dense phase search against
64 stand-alone soft read-outs of the 64 shifted contiguous crops, the window read-out against the per-unit read-out of the crop
regrouped on the host.  Against the NumPy statement (tests/_resync.py over tests/_svd_soft.py) a phase's score is within the summed
_svd_soft.unit_budget of its units."""
import numpy as np
import pytest

import offmark_oracle as orc
import _resync as rs

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
    """The contiguous crop holding the full units of phase (py, px) of a device batch, and its (rows, cols); None without a unit."""
    H, W = dev.shape[1:3]
    r, c = (H - py) // 8, (W - px) // 8
    if r < 1 or c < 1:
        return None, (r, c)
    return dev[:, py:py + 8 * r, px:px + 8 * c].contiguous(), (r, c)


SHAPES = {"leak-2x61x83": None, "1x100x139": (1, 100, 139), "1x8x8": (1, 8, 8), "1x8x40": (1, 8, 40), "1x40x9": (1, 40, 9)}


def frames_of(shape_id):
    if SHAPES[shape_id] is None:
        return np.array(rs.oracle_leak()[:2])
    n, H, W = SHAPES[shape_id]
    return np.stack([orc.synthetic_frame(H, W, 7000 + H + i) for i in range(n)])


# ---- 1. the dense phase search ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [15, 3.5])
@pytest.mark.parametrize("shape_id", list(SHAPES))
def test_scores_equal_the_soft_read_out_of_every_shifted_crop(eng, shape_id, scale):
    frames = frames_of(shape_id)
    dev = cuda(frames)
    n, H, W = frames.shape[:3]
    got = eng.svd_sync_scores(dev, scale=scale, scores=garbage(n, 64)).cpu().numpy()
    assert got.shape == (n, 64) and got.dtype == np.int64
    ref = np.zeros((n, 64), np.int64)
    for py in range(8):
        for px in range(8):
            crop, (r, c) = device_crop(dev, py, px)
            if crop is not None:
                ref[:, 8 * py + px] = eng.svd_detect_soft(crop, r * c, scale=scale).abs().sum(dim=1).cpu().numpy()
    from offmark import resync
    units = resync.units_per_phase(H, W)
    assert (got[:, units == 0] == 0).all() and (got[:, units > 0] > 0).all()   # a phase without units scores 0
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    if scale == 15:                                                            # ... and against the NumPy statement
        for f in range(n):
            want, budget = rs.statement_scores(frames[f], scale=15.0)
            d = np.abs(got[f] - want)
            print(f"{shape_id} frame {f}: worst |device - statement| {d.max()} (budget there {budget[d.argmax()]})")
            assert (d <= budget).all(), (f, d.max(), budget[d.argmax()])


def test_scores_of_frames_past_a_launch_chunk(eng):
    """More frames than one launch takes (65535): the second launch's frames and rows start where the first one's end."""
    import torch
    n, edge = 65537, 65535
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    frames = torch.randint(0, 256, (n, 8, 9, 3), dtype=torch.uint8, device="cuda", generator=g)
    full = eng.svd_sync_scores(frames, scores=garbage(n, 64))
    assert torch.equal(full[edge - 3:], eng.svd_sync_scores(frames[edge - 3:].contiguous()))
    assert torch.equal(full[:5], eng.svd_sync_scores(frames[:5].contiguous()))
    assert (full[:, :2] > 0).float().mean() > 0.9 and not full[:, 2:].any()     # an 8x9 frame has the phases (0, 0) and (0, 1)
    win = eng.svd_detect_soft_window(frames, 3, (0, 1), 5, base=2, soft=garbage(n, 3))
    assert torch.equal(win[edge - 3:], eng.svd_detect_soft_window(frames[edge - 3:].contiguous(), 3, (0, 1), 5, base=2))
    assert torch.equal(win[:, 2].abs(), full[:, 1]) and not win[:, :2].any()     # one unit per frame, at position (2 + 0) % 3


# ---- 2. the window read-out --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 29])
@pytest.mark.parametrize("phase", [(5, 3), (0, 0), (7, 7)])
def test_window_equals_the_crop_read_out_regrouped(eng, phase, base):
    dev = cuda(rs.oracle_leak())
    n = dev.shape[0]
    crop, (r, c) = device_crop(dev, *phase)
    per_unit = eng.svd_detect_soft(crop, r * c).cpu().numpy()
    assert (per_unit != 0).mean() > 0.9
    for L in (8, 5, 77, 3000):                                                 # 3000: past the LDS histogram
        got = eng.svd_detect_soft_window(dev, L, phase, 13, base=base, soft=garbage(n, L)).cpu().numpy()
        ref = np.stack([rs.canvas_regroup(per_unit[f], r, c, 13, base, L) for f in range(n)])
        assert got.shape == (n, L) and got.dtype == np.int64 and np.array_equal(got, ref), (L, np.argwhere(got != ref)[:5])


def test_window_at_the_origin_is_the_soft_read_out(eng):
    import torch
    H, W, n = 64, 96, 3
    dev = cuda(np.stack([orc.synthetic_frame(H, W, 7100 + i) for i in range(n)]))
    for L in (8, 5, 96, 3000):
        got = eng.svd_detect_soft_window(dev, L, (0, 0), W // 8, soft=garbage(n, L))
        assert torch.equal(got, eng.svd_detect_soft(dev, L)) and got.any()
    z = eng.svd_detect_soft_window(dev, 8, (0, 0), W // 8, scales=(10, 0, 20), soft=garbage(n, 8))
    assert z.shape == (n, 8) and not z.any()                                   # channel 1 unmarked: zeros, as the soft read-out


# ---- 3. end to end on the device ----------------------------------------------------------------------------------------------
def test_a_cropped_leak_is_read_end_to_end(eng):
    from offmark import resync
    from offmark.dist.vote import soft_vote
    from offmark.degenerator.de_shuffler import DeShuffler
    from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder
    from offmark.generator.shuffler import Shuffler
    pay, seg = rs.recipe_payloads(), rs.recipe_segments()
    wm = np.stack([Shuffler(key=rs.KEY).generate_wm(p, (rs.H * rs.W // 64,)) for p in pay]).astype(np.uint8)
    marked = eng.svd_embed(cuda(rs.recipe_sources()), wm, wm_row=cuda(seg.astype(np.int32)))
    leak = marked[:, rs.CROP[0]:, rs.CROP[1]:].contiguous()
    assert tuple(leak.shape) == (12, 61, 83, 3)
    got = resync.read_cropped_leak(DwtDctSvdDecoder(), leak, seg, rs.W, rs.recipe_candidates(), key=rs.KEY, L=rs.L8)
    print(f"phase {got['phase']} contrast {got['contrast']:.3f} base {got['base']} picks {list(got['picks'])} "
          f"score {got['score']} runner-up {got['runner_up_score']}")
    assert got["phase"] == rs.PHASE and got["base"] == rs.BASE and list(got["picks"]) == list(rs.CHOSEN) and not got["ambiguous"]
    assert got["contrast"] > 1.2
    # what the feature buys: the plain soft read-out of the same leak, cut to a multiple of 8 at phase (0, 0), read by sign
    plain = eng.svd_detect_soft(leak[:, :56, :80].contiguous(), rs.L8).cpu().numpy()
    by_sign = soft_vote(plain, DeShuffler(key=rs.KEY).set_shape((rs.L8,)).payload_idx, seg)
    right = sum(int(np.array_equal(by_sign[s], pay[s])) for s in range(rs.S))
    print(f"plain read-out at phase (0, 0): {right}/3 segments by sign")
    assert right < 3


# ---- 4. graph capture ----------------------------------------------------------------------------------------------------------
def test_both_calls_are_graph_capturable(eng):
    """No allocation and no synchronisation inside the calls: they capture into a HIP graph and replay with identical results."""
    import torch
    dev = cuda(rs.oracle_leak())
    n = dev.shape[0]
    ref_scores = eng.svd_sync_scores(dev)
    ref_soft = eng.svd_detect_soft_window(dev, 8, rs.PHASE, 13, base=3)
    torch.cuda.synchronize()
    scores, soft = garbage(n, 64), garbage(n, 8)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng.svd_sync_scores(dev, scores=scores)              # warm-up on the capture stream
        eng.svd_detect_soft_window(dev, 8, rs.PHASE, 13, base=3, soft=soft)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            eng.svd_sync_scores(dev, scores=scores)
            eng.svd_detect_soft_window(dev, 8, rs.PHASE, 13, base=3, soft=soft)
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
