"""GPU: reading rotated leaks (engine.warp_affine / svd_affine_scores / svd_detect_soft_affine, DwtDctSvdDecoder's affine methods,
offmark.resync.read_rescaled_leak with [K, 6] geometries; build extensions, not reference semantics).

The warp is defined in integers, so the device equals the NumPy statement (tests/_affine.py) byte for byte.  The fused calls are
held against the chain they replace -- warp_affine of the whole canvas, svd_detect_soft with one position per unit, the
statement's per-pixel counting units as the mask -- integer for integer, nothing else masked out; output buffers arrive filled
with garbage.  End to end the recipe is marked on the device and rotated on the host (tests/_affine.py: float64 bilinear)."""
import numpy as np
import pytest

import offmark_oracle as orc
import _affine as af
import _resync as rs
import _warp as wp

pytestmark = pytest.mark.gpu

ONE = af.ONE
CANVAS = af.CANVAS                           # 72 x 104: 9 x 13 units, one (partial) workgroup tile of the search
UNITS = (CANVAS[0] // 8) * (CANVAS[1] // 8)
NO_UNIT = (ONE, 0, 1 << 40, 0, ONE, 0)
OUT_OF_RANGE = (ONE, ONE, 0, ONE, ONE, 0)                    # singular
ONE_UNIT = (ONE, 0, -(58 << 16), 0, ONE, -(90 << 16))        # of a 61 x 83 leak only canvas unit (8, 12) is wholly inside
SHEAR = (ONE, 8192, 0, 0, ONE, 0)


def turn(w):
    """A quarter turn: canvas (y, x) reads leak (x, w - 1 - y)."""
    return 0, ONE, 0, -ONE, 0, (w - 1) << 16


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
def rot72():
    """5 frames of the oracle-marked recipe rotated by 2 degrees about the centre, 72 x 104."""
    return np.array(af.leak("svd")[:5])


def rotation(leak_hw, angle, scale=1.0, shift=(0.0, 0.0), canvas=CANVAS):
    from offmark import resync
    return resync.affine_of_rotation(canvas, leak_hw, angle, scale, shift)


def geometries(leak_hw):
    """The named maps of the warp test for a leak of this size."""
    h, w = leak_hw
    return {"2deg": rotation(leak_hw, 2.0), "-3deg-step-1.10": rotation(leak_hw, -3.0, 1.10), "hflip": af.hflip(w), "turn": turn(w),
            "shear": SHEAR, "half-turn": (-ONE, 0, (h - 1) << 16, 0, -ONE, (w - 1) << 16)}


chain_unit_metrics = af.chain_unit_metrics       # warp_affine of the whole canvas + svd_detect_soft, masked by the statement's units


# ---- 1. the warp against the statement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("which", ["leak61", "rot72"])
def test_warp_equals_the_statement(eng, request, which, n):
    import torch
    frames = request.getfixturevalue(which)[:n]
    for name, g in geometries(frames.shape[1:3]).items():
        for out_hw, origin in ((CANVAS, (0, 0)), ((37, 45), (8, 16))):
            got = eng.warp_affine(cuda(frames), g, out_hw, origin=origin, out=garbage((n, *out_hw, 3), torch.uint8)).cpu().numpy()
            ref = np.stack([af.warp(f, g, out_hw, origin)[0] for f in frames])
            assert got.shape == ref.shape and got.dtype == np.uint8 and np.array_equal(got, ref), (name, np.argwhere(got != ref)[:5])
            assert ref.any()
    h, w = frames.shape[1:3]
    assert np.array_equal(eng.warp_affine(cuda(frames), af.hflip(w), (h, w)).cpu().numpy(), frames[:, :, ::-1])      # the mirrored frame


def test_warp_at_zero_off_diagonals_is_the_axis_aligned_warp(eng, leak61):
    import torch
    from offmark import resync
    dev = cuda(leak61)
    for g4, out_hw, origin in ((wp.true_geometry((61, 83)), CANVAS, (0, 0)), ((49152, -8192, 98304, 16384), (85, 61), (3, 2)),
                               (wp.IDENTITY, (61, 83), (0, 0))):
        assert torch.equal(eng.warp_affine(dev, resync.affine_of_warp(g4), out_hw, origin=origin), eng.warp(dev, g4, out_hw, origin=origin))


# ---- 2. the fused scores against the chain --------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [15, 3.5])
def test_scores_equal_the_chain_over_the_35_candidates(eng, rot72, scale):
    dev = cuda(rot72)
    n = dev.shape[0]
    cands = af.candidate_geometries()
    got = eng.svd_affine_scores(dev, CANVAS, cands, scale=scale, scores=garbage((n, len(cands)))).cpu().numpy()
    assert got.shape == (n, 35) and got.dtype == np.int64
    ref = np.stack([np.abs(chain_unit_metrics(eng, dev, CANVAS, g, scale)).sum(axis=(1, 2)) for g in cands], axis=1)
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    assert (got > 0).all()


@pytest.mark.parametrize("n", [1, 5])
def test_scores_on_the_odd_leak_and_scores_of_zero(eng, leak61, n):
    """61 x 83: rows of 249 bytes, so a pixel's 6-byte tap pairs start at every alignment.  A candidate out of range and one
    without a unit score 0 while their neighbours do not change."""
    dev = cuda(leak61[:n])
    named = geometries((61, 83))
    cands = np.array([named["2deg"], OUT_OF_RANGE, named["-3deg-step-1.10"], NO_UNIT, named["hflip"], named["turn"], SHEAR, ONE_UNIT,
                      named["half-turn"], (1 << 21, 0, 0, 0, ONE, 0), rotation((61, 83), 31.0, 0.8)], np.int64)
    got = eng.svd_affine_scores(dev, CANVAS, cands, scores=garbage((n, len(cands)))).cpu().numpy()
    ref = np.zeros_like(got)
    for k, g in enumerate(cands):
        if k not in (1, 9):                                                    # out of range: the host calls refuse these maps
            ref[:, k] = np.abs(chain_unit_metrics(eng, dev, CANVAS, g)).sum(axis=(1, 2))
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    assert not got[:, [1, 3, 9]].any() and (np.delete(got, [1, 3, 9], axis=1) > 0).all()
    assert af.units((61, 83), CANVAS, ONE_UNIT).sum() == 1
    alone = eng.svd_affine_scores(dev, CANVAS, cands[[0, 2, 4]]).cpu().numpy()
    assert np.array_equal(alone, got[:, [0, 2, 4]])


def test_scores_at_zero_off_diagonals_are_the_warp_scores(eng, leak61):
    import torch
    from offmark import resync
    dev = cuda(leak61)
    c4 = np.array([wp.IDENTITY, (ONE, -(11 << 16), ONE, -(21 << 16)), (49152, -8192, 49152, -8192), (98304, 16384, 98304, 16384),
                   (ONE, 1 << 40, ONE, 0), wp.true_geometry((61, 83))], np.int64)
    c6 = np.array([resync.affine_of_warp(g) for g in c4], np.int64)
    got = eng.svd_affine_scores(dev, CANVAS, torch.from_numpy(c6).cuda())      # a device tensor is taken as it is
    assert torch.equal(got, eng.svd_warp_scores(dev, CANVAS, c4)) and got[:, :4].all()


def test_a_leak_one_pixel_wide_or_high(eng):
    """w = 1 has no pixel pair to fetch and h = 1 no second row: upscaled 16 x, such a leak still fills canvas units."""
    import torch
    from offmark import resync
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    for leak_hw, g4 in (((20, 1), (ONE, 0, 4096, 0)), ((1, 30), (4096, 100, ONE, -(3 << 16)))):
        dev = torch.randint(0, 256, (2, *leak_hw, 3), dtype=torch.uint8, device="cuda", generator=g)
        c6 = np.array([resync.affine_of_warp(g4)], np.int64)
        got = eng.svd_affine_scores(dev, (16, 24), c6, scores=garbage((2, 1)))
        assert torch.equal(got, eng.svd_warp_scores(dev, (16, 24), np.array([g4], np.int64))) and got.all()
        assert int(af.units(leak_hw, (16, 24), c6[0]).sum()) == 4
        soft = eng.svd_detect_soft_affine(dev, (16, 24), c6[0], 6, soft=garbage((2, 6)))
        assert torch.equal(soft, eng.svd_detect_soft_warp(dev, (16, 24), g4, 6)) and soft.any()


def test_scores_over_many_tiles(eng):
    """A 33 x 49 unit canvas is 3 x 4 workgroup tiles: partial tiles, tiles that hold no counting unit and tiles that lie wholly
    beyond an edge of the small leak (they leave early).  Under the last two candidates a canvas pixel steps 2.2 leak pixels."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    canvas = (264, 392)
    small = torch.randint(0, 256, (2, 90, 131, 3), dtype=torch.uint8, device="cuda", generator=g)
    big = torch.randint(0, 256, (2, 301, 433, 3), dtype=torch.uint8, device="cuda", generator=g)
    for dev, params in ((small, [(4.0, 1.0), (-2.0, 0.9), (90.0, 1.0), (0.0, 1.0)]), (big, [(3.0, 1.0), (-7.5, 1.3), (12.0, 1 / 2.2), (-1.0, 1 / 2.2)])):
        leak_hw = tuple(dev.shape[1:3])
        cands = np.array([rotation(leak_hw, a, s, canvas=canvas) for a, s in params], np.int64)
        got = eng.svd_affine_scores(dev, canvas, cands, scores=garbage((2, len(cands)))).cpu().numpy()
        ref = np.stack([np.abs(chain_unit_metrics(eng, dev, canvas, c)).sum(axis=(1, 2)) for c in cands], axis=1)
        assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]
        assert (got > 0).all()


def test_scores_of_candidates_past_a_launch_chunk(eng):
    """More candidates than one launch takes (65535 sit in gridDim.y): the entries past the chunk equal the same candidates scored
    alone.  A 16 x 24 leak on a 16 x 24 canvas, n = 1: small rotations and sub-pixel shifts that keep units inside."""
    import torch
    K, edge = 65535 + 3, 65535
    g = torch.Generator(device="cuda")
    g.manual_seed(12)
    frames = torch.randint(0, 256, (1, 16, 24, 3), dtype=torch.uint8, device="cuda", generator=g)
    k = np.arange(K, dtype=np.int64)
    skew = 16 * (k % 61) - 480                                                 # off-diagonals up to +-480 / 65536: 0.4 degrees
    cands = np.stack([np.full(K, ONE), skew, 7 * (k % 251), -skew, np.full(K, ONE), 5 * (k % 241)], axis=1)
    dev_cands = torch.from_numpy(cands).cuda()
    full = eng.svd_affine_scores(frames, (16, 24), dev_cands, scores=garbage((1, K)))
    assert torch.equal(full[:, edge - 3:], eng.svd_affine_scores(frames, (16, 24), dev_cands[edge - 3:].contiguous()))
    assert torch.equal(full[:, :5], eng.svd_affine_scores(frames, (16, 24), dev_cands[:5].contiguous()))
    assert (full > 0).float().mean() > 0.9
    for kk in (edge - 1, edge, K - 1):
        assert int(full[0, kk]) == int(np.abs(chain_unit_metrics(eng, frames, (16, 24), cands[kk])).sum()), kk


# ---- 3. the fused read-out against the chain --------------------------------------------------------------------------------------
def chain_soft(eng, dev, g, L):
    m = chain_unit_metrics(eng, dev, CANVAS, g)
    return np.stack([af.ss.regroup(f.reshape(-1), L) for f in m])


@pytest.mark.parametrize("which,name", [("rot72", "2deg"), ("leak61", "2deg"), ("leak61", "-3deg-step-1.10"), ("leak61", "turn"), ("leak61", "one-unit")])
def test_read_out_equals_the_chain(eng, request, which, name):
    dev = cuda(request.getfixturevalue(which))
    n = dev.shape[0]
    g = ONE_UNIT if name == "one-unit" else geometries(tuple(dev.shape[1:3]))[name]
    assert (af.units(tuple(dev.shape[1:3]), CANVAS, g).sum() == 1) == (name == "one-unit")
    for L in (8, UNITS, 3000):                                                 # 3000: past the LDS histogram
        got = eng.svd_detect_soft_affine(dev, CANVAS, g, L, soft=garbage((n, L)))
        assert got.shape == (n, L) and np.array_equal(got.cpu().numpy(), chain_soft(eng, dev, g, L)), L
        assert got.any()
    z = eng.svd_detect_soft_affine(dev, CANVAS, NO_UNIT, 8, soft=garbage((n, 8)))
    assert not z.any()                                                         # no counting unit: zeros, not an error
    z = eng.svd_detect_soft_affine(dev, CANVAS, g, 8, scales=(10, 0, 20), soft=garbage((n, 8)))
    assert not z.any()                                                         # channel 1 unmarked: zeros, as the soft read-out


def test_read_out_at_zero_off_diagonals_and_at_the_identity(eng, leak61):
    import torch
    from offmark import resync
    dev = cuda(leak61)
    for g4 in ((ONE, -(11 << 16), ONE, -(21 << 16)), (49152, -8192, 49152, -8192), wp.true_geometry((61, 83))):
        for L in (8, 5):
            got = eng.svd_detect_soft_affine(dev, CANVAS, resync.affine_of_warp(g4), L)
            assert torch.equal(got, eng.svd_detect_soft_warp(dev, CANVAS, g4, L)) and got.any()
    whole = cuda(np.stack([orc.synthetic_frame(wp.H, wp.W, 7200 + i) for i in range(3)]))
    for L in (8, 5):
        got = eng.svd_detect_soft_affine(whole, CANVAS, af.IDENTITY, L)
        assert torch.equal(got, eng.svd_detect_soft(whole, L)) and got.any()


# ---- 4. end to end on the device ------------------------------------------------------------------------------------------------
def device_marked(eng):
    """The recipe marked ON THE DEVICE (one watermark row per segment), back on the host: u8 [12, 72, 104, 3]."""
    from offmark.generator.shuffler import Shuffler
    pay, seg = rs.recipe_payloads(), rs.recipe_segments()
    wm = np.stack([Shuffler(key=af.KEY).generate_wm(p, (af.H * af.W // 64,)) for p in pay]).astype(np.uint8)
    return eng.svd_embed(cuda(rs.recipe_sources()), wm, wm_row=cuda(seg.astype(np.int32))).cpu().numpy()


def test_a_rotated_leak_is_found_and_read(eng):
    from offmark import resync
    from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder
    leak = cuda(af.rotate(device_marked(eng), *af.ATTACKS["2deg"]))
    cands = af.candidate_geometries()
    got = resync.read_rescaled_leak(DwtDctSvdDecoder(), leak, rs.recipe_segments(), CANVAS, rs.recipe_candidates(), cands, key=af.KEY,
                                    L=af.L8, search_frames=af.SEARCH_FRAMES)
    n = got["normalised"]
    print(f"index {got['index']} true {n[0]:.4f} best other {np.delete(n, 0).max():.4f} contrast {got['contrast']:.4f} picks {[int(p) for p in got['picks']]}")
    assert got["index"] == 0 and got["geometry"] == tuple(cands[0])
    assert list(got["picks"]) == list(af.CHOSEN) and not got["ambiguous"] and got["base"] == 0


def test_the_dct_decoder_refuses_an_affine_geometry(eng, rot72):
    from offmark import resync
    from offmark.extract.dct_decoder import DctDecoder
    for geoms in (af.candidate_geometries(), af.candidate_geometries()[:1]):
        with pytest.raises(ValueError, match="affine"):
            resync.read_rescaled_leak(DctDecoder(alpha=20), cuda(rot72), rs.recipe_segments()[:5], CANVAS, rs.recipe_candidates(), geoms)


# ---- 5. graph capture -----------------------------------------------------------------------------------------------------------
def test_all_three_calls_are_graph_capturable(eng, rot72):
    """No allocation and no synchronisation inside the calls: they capture into a HIP graph on one stream (no parallel branches)
    and replay with identical results."""
    import torch
    dev = cuda(rot72)
    n = dev.shape[0]
    cands = torch.from_numpy(af.candidate_geometries()[:7]).cuda()
    g = tuple(int(v) for v in af.candidate_geometries()[0])
    ref_warp = eng.warp_affine(dev, g, (70, 99), origin=(1, 2))
    ref_scores = eng.svd_affine_scores(dev, CANVAS, cands)
    ref_soft = eng.svd_detect_soft_affine(dev, CANVAS, g, 8)
    torch.cuda.synchronize()
    out, scores, soft = garbage((n, 70, 99, 3), torch.uint8), garbage((n, 7)), garbage((n, 8))
    stream = torch.cuda.Stream()

    def calls():
        eng.warp_affine(dev, g, (70, 99), origin=(1, 2), out=out)
        eng.svd_affine_scores(dev, CANVAS, cands, scores=scores)
        eng.svd_detect_soft_affine(dev, CANVAS, g, 8, soft=soft)

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
    assert ref_scores.all() and ref_soft.any()
    del graph
    import gc
    gc.collect()
    torch.cuda.synchronize()
