"""GPU: the dense shift search under an affine map (engine.svd_affine_phase_scores, DwtDctSvdDecoder.affine_phase_scores_u8,
offmark.resync.read_transformed_leak; build extensions, not reference semantics).

The call is defined by what exists: entry [f][k][8 py + px] is engine.svd_affine_scores of frame f under
offmark.resync.shift_affine(cands[k], py, px), and units[k][8 py + px] is engine.affine_units' count of that geometry -- held
integer for integer, nothing masked out; output buffers arrive filled with garbage.  One frame is also held against the NumPy
statement (tests/_affine_phase.py) within the project's float32 budget per unit.  End to end the recipe is marked on the device,
rotated on the host (tests/_affine.py: float64 bilinear) and cropped off-centre."""
import numpy as np
import pytest

import _affine as af
import _affine_phase as ap
import _resync as rs

pytestmark = pytest.mark.gpu

ONE = af.ONE
CANVAS = ap.CANVAS                           # 72 x 104 pixel origins: 3 x 4 workgroup rectangles, the last of each partial
N = 3
ZEROS = (0, 0, 0, 0, 0, 0)                   # out of range: singular
OUTSIDE = (ONE, 0, 1 << 40, 0, ONE, 0)       # in range, the leak wholly outside the canvas


@pytest.fixture(scope="module")
def eng():
    import torch
    from offmark.engine import DctEngine
    torch.cuda.set_device(0)
    return DctEngine()


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the shared references are read-only


def garbage(shape):
    """The output buffer a call gets holds anything non-zero: the library clears all of it."""
    import torch
    return torch.full(shape, 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")


def rotation(leak_hw, angle, scale=1.0, shift=(0.0, 0.0), canvas=CANVAS):
    from offmark import resync
    return resync.affine_of_rotation(canvas, leak_hw, angle, scale, shift)


def six(leak_hw, canvas=CANVAS):
    """K = 6: the truth of a leak rotated by 2 degrees, an angle off, a half-pixel shift, a zero-off-diagonal map, the horizontal
    flip and one out-of-range candidate."""
    return np.array([rotation(leak_hw, 2.0, canvas=canvas), rotation(leak_hw, 2.5, canvas=canvas), rotation(leak_hw, 2.0, 1.0, (0.5, 0.5), canvas),
                     (60000, 0, 3 << 15, 0, 70000, -(5 << 14)), af.hflip(leak_hw[1]), ZEROS], np.int64)


def leak_frames(leak_hw):
    """3 frames of 57 x 91 (leak B: the recipe rotated and cropped) or of 61 x 83 (the cropped recipe): odd widths, unaligned rows."""
    return np.array(ap.leak("svd", "B")[:N] if leak_hw == (57, 91) else rs.oracle_leak()[:N])


def reference(eng, dev, canvas, cands, scale=15):
    """(scores [n, K, 64], units [K, 64]) on the host from the calls that exist: svd_affine_scores over the 64 K shifted candidates
    (it scores an out-of-range one 0) and the host-only affine_units of each (which refuses one: 0 units)."""
    from offmark import resync
    K = len(cands)
    shifted = np.stack([resync.shift_affine(cands, py, px) for py in range(8) for px in range(8)], axis=1)      # [K, 64, 6]
    scores = eng.svd_affine_scores(dev, canvas, shifted.reshape(K * 64, 6), scale=scale).cpu().numpy().reshape(-1, K, 64)
    units = np.zeros((K, 64), np.int64)
    for k in range(K):
        if ap.in_range(cands[k]):
            units[k] = [eng.affine_units(tuple(dev.shape[1:3]), canvas, g)[4] for g in shifted[k]]
        else:
            scores[:, k] = 0                       # some of its 64 shifts may be in range alone: the call defines all 64 as 0
    return scores, units


def check(eng, dev, canvas, cands, scale=15):
    n, K = dev.shape[0], len(cands)
    scores, units = eng.svd_affine_phase_scores(dev, canvas, cands, scale=scale, scores=garbage((n, K, 64)), units=garbage((K, 64)))
    assert scores.shape == (n, K, 64) and units.shape == (K, 64) and scores.dtype == units.dtype
    got, got_units = scores.cpu().numpy(), units.cpu().numpy()
    assert got.dtype == np.int64
    ref, ref_units = reference(eng, dev, canvas, cands, scale)
    assert np.array_equal(got_units, ref_units), np.argwhere(got_units != ref_units)[:5]
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    assert ((got > 0) == (ref_units > 0)[None]).all()
    return got, got_units


# ---- 1. against the calls that exist ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leak_hw", [(57, 91), (61, 83)])
def test_scores_and_units_equal_the_64_shifted_candidates(eng, leak_hw):
    dev = cuda(leak_frames(leak_hw))
    assert tuple(dev.shape) == (N, *leak_hw, 3)
    cands = six(leak_hw)
    got, units = check(eng, dev, CANVAS, cands)
    assert not got[:, 5].any() and not units[5].any() and (units[:5].max(axis=1) > 20).all()
    assert len({int(u) for u in units[0]}) > 4                                 # the count depends on the shift
    check(eng, dev, CANVAS, cands[[2, 4]], scale=3.5)
    # a candidate in range alone but out of range under its last shifts: zeros in all 64 entries
    edge = np.array([cands[0], (ONE, 0, (1 << 48) - 3 * ONE, 0, ONE, 0)], np.int64)
    assert not ap.in_range(edge[1])
    check(eng, dev, CANVAS, edge)


@pytest.mark.parametrize("canvas", [(32, 32), (40, 8), (8, 40), (45, 70)])
def test_small_canvases(eng, canvas):
    """32 x 32 is exactly one rectangle of origins; 40 x 8 a single column of units over two rectangles, 8 x 40 a single row; 45 x 70
    holds 5 x 8 units and 5 rows and 6 columns of pixels that belong to none.  Shifted units reach past the canvas's last row and
    column: canvas coordinates are an index space."""
    dev = cuda(leak_frames((57, 91)))
    cands = np.array([af.IDENTITY, rotation((57, 91), 2.0, canvas=canvas), rotation((57, 91), -30.0, 0.5, (0.5, 0.25), canvas), af.hflip(91), ZEROS], np.int64)
    got, units = check(eng, dev, canvas, cands)
    assert (units[0] == (canvas[0] // 8) * (canvas[1] // 8)).all() and got[:, [0, 1, 3]].all()


def test_candidates_past_a_launch_chunk(eng):
    """More candidates than one launch takes (65535 sit in gridDim.y): rows 65533.. (two before the chunk edge, two past it) and a
    strided sample of the earlier rows, scores and units, equal the same candidates in a call of their own, so the second launch's
    candidate offset and both output offsets (* 64) are right.  The 40 x 8 canvas of test_small_canvases under a 48 x 16 leak, which
    holds every shifted unit; n = 1: the identity with sub-pixel offsets, four distinct small shears around the edge.  The frame side
    of the chunk rule (launches of fewer frames once n * K workgroups pass 2^30) is not tested: it needs n * K >= 2^30 outputs."""
    import torch
    K, edge, canvas = 65535 + 2, 65535, (40, 8)
    g = torch.Generator(device="cuda")
    g.manual_seed(21)
    frames = torch.randint(0, 256, (1, 48, 16, 3), dtype=torch.uint8, device="cuda", generator=g)
    k = np.arange(K, dtype=np.int64)
    cands = np.stack([np.full(K, ONE), 0 * k, 3 * (k % 251), 0 * k, np.full(K, ONE), 5 * (k % 241)], axis=1)
    cands[edge - 2:] = [(ONE, s, 1 << 15, -s, ONE, 1 << 16) for s in (200, 400, 600, 800)]
    cands = torch.from_numpy(cands).cuda()
    full, full_units = eng.svd_affine_phase_scores(frames, canvas, cands, scores=garbage((1, K, 64)), units=garbage((K, 64)))
    for rows in (slice(edge - 2, K), torch.arange(0, edge - 2, 4099, device="cuda")):
        own, own_units = eng.svd_affine_phase_scores(frames, canvas, cands[rows].contiguous())
        assert torch.equal(full[:, rows], own) and torch.equal(full_units[rows], own_units)
    assert (full_units[:edge - 2] == 5).all() and (full_units[edge:] > 0).all() and full[0, edge:].any(dim=1).all()


def test_a_canvas_larger_than_the_leak(eng):
    """136 x 200 pixel origins are 5 x 7 rectangles over a 57 x 91 leak: rectangles wholly beyond an edge of the leak (they leave
    early), rectangles the leak's edge runs through, and under the last candidate (a canvas pixel steps 2.2 leak pixels) only a
    few units in the middle."""
    dev = cuda(leak_frames((57, 91)))
    canvas = (136, 200)
    cands = np.array([af.IDENTITY, rotation((57, 91), 4.0, canvas=canvas), (ONE, 0, -(70 << 16), 0, ONE, -(100 << 16)),
                      rotation((57, 91), -7.5, 1 / 2.2, (0.5, 0.0), canvas)], np.int64)
    got, units = check(eng, dev, canvas, cands)
    assert got.any(axis=(0, 2)).all() and (units.max(axis=1) < 17 * 25).all()


def test_nothing_counts(eng):
    """A leak smaller than one unit and a map that puts the leak wholly outside the canvas: zeros for scores and units."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    tiny = torch.randint(0, 256, (N, 5, 6, 3), dtype=torch.uint8, device="cuda", generator=g)
    got, units = check(eng, tiny, CANVAS, np.array([af.IDENTITY, rotation((5, 6), 2.0)], np.int64))
    assert not got.any() and not units.any()
    dev = cuda(leak_frames((61, 83)))
    got, units = check(eng, dev, CANVAS, np.array([OUTSIDE, (ONE, 0, 0, 0, ONE, -(1 << 40))], np.int64))
    assert not got.any() and not units.any()


# ---- 2. against the NumPy statement -----------------------------------------------------------------------------------------------
def test_one_frame_against_the_statement(eng):
    """Units exactly; a score within the summed float32 budget of its units (tests/_svd_soft.py: unit_budget)."""
    frame = leak_frames((57, 91))[1:2]
    cands = six((57, 91))[[2, 4]]                                               # K = 2: the half-pixel shift and the flip
    scores, units = eng.svd_affine_phase_scores(cuda(frame), CANVAS, cands)
    want, want_units = ap.statement_scores(frame, CANVAS, cands)
    assert np.array_equal(units.cpu().numpy(), want_units) and want_units.any()
    d = np.abs(scores.cpu().numpy() - want)[0]
    budget = np.stack([ap.statement_budget(frame[0], CANVAS, tuple(int(v) for v in g)) for g in cands])
    print(f"worst |device - statement| {d.max()} (budget there {budget.reshape(-1)[d.argmax()]}, smallest budget {budget[want_units > 0].min()})")
    assert (d <= budget).all(), (d.max(), budget.reshape(-1)[d.argmax()])


# ---- 3. the outputs -----------------------------------------------------------------------------------------------------------------
def test_units_may_be_left_out_and_buffers_are_cleared(eng):
    import torch
    dev = cuda(leak_frames((57, 91)))
    cands = torch.from_numpy(six((57, 91))).cuda()                             # a device tensor is taken as it is
    ref, ref_units = eng.svd_affine_phase_scores(dev, CANVAS, cands)
    assert ref.any() and ref_units.any()
    scores, none = eng.svd_affine_phase_scores(dev, CANVAS, cands, scores=garbage((N, 6, 64)), units=False)      # units = NULL
    assert none is None and torch.equal(scores, ref)
    # every entry without a counting unit was garbage and is 0 now; calling again into the same buffers adds nothing
    buf, ubuf = garbage((N, 6, 64)), garbage((6, 64))
    for _ in range(2):
        s, u = eng.svd_affine_phase_scores(dev, CANVAS, cands, scores=buf, units=ubuf)
        assert s is buf and u is ubuf and torch.equal(buf, ref) and torch.equal(ubuf, ref_units)
    assert not buf[:, 5].any() and not ubuf[5].any()
    # one frame, and frames 1.. alone: units do not depend on the frames, scores are per frame
    s1, u1 = eng.svd_affine_phase_scores(dev[1:], CANVAS, cands)
    assert torch.equal(s1, ref[1:]) and torch.equal(u1, ref_units)
    with pytest.raises(ValueError):
        eng.svd_affine_phase_scores(dev, CANVAS, six((57, 91))[:, :4])
    with pytest.raises(ValueError):
        eng.svd_affine_phase_scores(dev, CANVAS, cands, units=garbage((6, 63)))


def test_the_call_is_graph_capturable(eng):
    """No allocation and no synchronisation inside the call: it captures into a HIP graph on one stream (no parallel branches) and
    replays with identical results."""
    import torch
    dev = cuda(leak_frames((57, 91)))
    cands = torch.from_numpy(six((57, 91))).cuda()
    ref, ref_units = eng.svd_affine_phase_scores(dev, CANVAS, cands)
    torch.cuda.synchronize()
    scores, units = garbage((N, 6, 64)), garbage((6, 64))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng.svd_affine_phase_scores(dev, CANVAS, cands, scores=scores, units=units)      # warm-up on the capture stream
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            eng.svd_affine_phase_scores(dev, CANVAS, cands, scores=scores, units=units)
    scores.fill_(7)
    units.fill_(7)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(scores, ref) and torch.equal(units, ref_units) and ref.any()
    del graph
    import gc
    gc.collect()
    torch.cuda.synchronize()


# ---- 4. end to end on the device ----------------------------------------------------------------------------------------------------
def device_marked(eng):
    """The recipe marked ON THE DEVICE (one watermark row per segment), back on the host: u8 [12, 72, 104, 3]."""
    from offmark.generator.shuffler import Shuffler
    pay, seg = rs.recipe_payloads(), rs.recipe_segments()
    wm = np.stack([Shuffler(key=af.KEY).generate_wm(p, (af.H * af.W // 64,)) for p in pay]).astype(np.uint8)
    return eng.svd_embed(cuda(rs.recipe_sources()), wm, wm_row=cuda(seg.astype(np.int32))).cpu().numpy()


def test_a_rotated_and_cropped_leak_is_found_and_read(eng):
    from offmark import resync
    from offmark.extract.dct_decoder import DctDecoder
    from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder
    (r0, r1), (c0, c1), _ = ap.LEAKS["B"]
    leak = cuda(af.rotate(device_marked(eng), *af.ATTACKS["2deg"])[:, r0:r1, c0:c1])
    cands = ap.candidates("B")
    got = ap.read(DwtDctSvdDecoder(), leak, cands)
    n = got["normalised"]
    print(f"index {got['index']} phase {got['phase']} normalised {n.max():.4f} contrast {got['contrast']:.4f} phase contrast "
          f"{got['phase_contrast']:.4f} picks {[int(p) for p in got['picks']]} base {got['base']}")
    assert list(got["picks"]) == list(af.CHOSEN) == [1, 0, 1] and not got["ambiguous"]
    assert got["index"] == 0 and got["phase"] == ap.TRUE_PHASE and got["geometry"] == resync.shift_affine(cands[0], 1, 2)
    with pytest.raises(ValueError, match="affine"):
        ap.read(DctDecoder(alpha=20), leak, cands)
