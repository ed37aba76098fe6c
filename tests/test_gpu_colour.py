"""GPU: the colour calls (engine.colour_sums / apply_colour, DwtDctSvdDecoder.colour_sums_u8 / apply_colour_u8,
offmark.colour.read_coloured_leak; build extensions, not reference semantics).

Everything is an integer, so the device is held against the NumPy statement (tests/_colour.py) exactly, nothing masked out; output
buffers arrive filled with garbage.  End to end the real decoder and the StatementDecoder see the same bytes, hence the same
histograms and sums, and the host arithmetic between the calls is the same: the table, the matrix and the geometries are the same."""
import functools

import numpy as np
import pytest

import _affine as af
import _affine_phase as ap
import _colour as co
import _resync as rs

pytestmark = pytest.mark.gpu

ONE = af.ONE
CANVAS = ap.CANVAS                           # 72 x 104: 2 x 2 tiles of 64 x 64 canvas pixels, the last of each partial
ZEROS = (0, 0, 0, 0, 0, 0)                   # out of range: singular
PART = (ONE, 0, 30 << 16, 0, ONE, 40 << 16)  # canvas (y, x) reads leak (y + 30, x + 40): a 26 x 50 corner of the canvas is inside
NONE = (ONE, 0, -(300 << 16), 0, ONE, 0)     # in range, and every canvas pixel reads above the leak's first row: nothing is inside
SHEAR = (ONE, 300, -(1 << 14), -200, ONE, -(1 << 15))      # sub-pixel offsets and a small shear: four taps per pixel, the first row and column outside


@functools.lru_cache(maxsize=None)
def registered():
    """What register_leak returns for leak A on the statement: about 0.1 px from the truth."""
    from offmark import resync
    return resync.register_leak(co.StatementDecoder(), rs.recipe_sources()[:ap.SEARCH_FRAMES], ap.leak("svd", "A")[:ap.SEARCH_FRAMES], CANVAS)["geometry"]


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
    import torch
    return torch.full(shape, 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def odd(a, offset=1):
    """The array on the device, starting ``offset`` bytes into its buffer."""
    import torch
    a = np.asarray(a)
    buf = torch.zeros(a.size + 8, dtype=torch.uint8, device="cuda")
    v = buf[offset:offset + a.size].view(a.shape)
    v.copy_(cuda(a))
    assert v.data_ptr() % 2 == 1 and v.is_contiguous()
    return v


# ---- 1. colour sums -----------------------------------------------------------------------------------------------------------------
def check_sums(eng, sources, frames, cands, dev=None):
    n, K = len(frames), len(cands)
    buf = garbage((n, K, 28))                                # pre-filled: the call clears it
    s, f = (cuda(sources), cuda(frames)) if dev is None else dev
    got = eng.colour_sums(s, f, np.asarray(cands, np.int64), sums=buf)
    assert got is buf
    got, want = got.cpu().numpy(), co.statement_sums(sources, frames, cands)
    assert got.shape == want.shape == (n, K, 28)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    return want


def test_sums_equal_the_statement_on_the_recipe(eng):
    """Leak A's 56 x 90 frames on the 72 x 104 canvas, n = 2, K = 5: the registered geometry, the unrotated start, a flip, one that
    covers a corner of the canvas only (three of the four tiles leave early or hold few pixels), one out of range; then the same leak
    colour-mapped (more clipped pixels, other products) and at odd addresses."""
    from offmark import resync
    frames, sources = ap.leak("svd", "A")[:2], rs.recipe_sources()[:2]
    assert ap.leak_hw("A") == (56, 90)
    cands = [registered(), resync.affine_of_rotation(CANVAS, (56, 90), 0.0), af.hflip(90), PART, ZEROS]
    want = check_sums(eng, sources, frames, cands)
    assert (want[:, 0, 0] > 3000).all()                      # of 56 * 90 = 5040; the first frame has 1587 clipped pixels
    assert (want[:, 3, 0] <= 26 * 50).all() and (want[:, 3, 0] > 1000).all() and not want[:, 4].any()
    mapped = co.colour_map(frames, *co.ATTACKS["hue+10-sat-1.2-gain-1.10-8"])
    more = check_sums(eng, sources, mapped, cands)
    assert (more[:, 0, 0] < want[:, 0, 0]).all()              # the saturation clips pixels, and they are left out
    check_sums(eng, sources, mapped, cands[:2], dev=(odd(sources, 1), odd(mapped, 3)))


@pytest.mark.parametrize("hw", [(8, 8), (64, 64), (65, 65), (130, 130)])
def test_sums_on_canvases_of_a_fraction_of_a_tile_one_tile_and_several(eng, hw):
    """h = H, w = W: under the identity every canvas pixel is inside and the warped bytes are the leak's; the shear reads four taps per
    pixel and leaves a strip outside; PART covers a corner or nothing (8 x 8); NONE is in range and covers nothing.  8 x 8 is a fraction
    of a tile, 64 x 64 exactly one, 65 x 65 has a last tile row of one pixel row and a last tile column of one pixel column, 130 x 130
    is 3 x 3 tiles.  Noise holds 0 and 255 in about 2 % of the pixels: they are left out."""
    frames, sources = noise((2, *hw, 3), 13), noise((2, *hw, 3), 14)
    want = check_sums(eng, sources, frames, [af.IDENTITY, SHEAR, PART, NONE, ZEROS])
    clipped = ((frames == 0) | (frames == 255)).any(axis=3).sum(axis=(1, 2))
    assert (clipped > 0).all() and np.array_equal(want[:, 0, 0], hw[0] * hw[1] - clipped)
    assert (want[:, 1, 0] > 0).all() and (want[:, 1, 0] < hw[0] * hw[1]).all()
    inside = max(hw[0] - 30, 0) * max(hw[1] - 40, 0)
    assert ((want[:, 2, 0] > 0) == (inside > 0)).all() and (want[:, 2, 0] <= inside).all() and not want[:, 3:].any()
    x = frames[0].reshape(-1, 3)[~((frames[0] == 0) | (frames[0] == 255)).any(axis=2).reshape(-1)].astype(np.int64)
    assert np.array_equal(want[0, 0, 1:4], x.sum(axis=0)) and want[0, 0, 8] == (x[:, 0] * x[:, 1]).sum()


def test_sums_of_full_tiles_at_the_largest_values(eng):
    """A whole 64 x 64 tile of leak 254 against source 255 under the identity: the largest sums a tile can have, 4096 * 254 * 255 =
    265 297 920 and 4096 * 255 * 255 = 266 342 400, just below 2^28, carried in 32 unsigned bits through the wavefront and LDS.  On a
    320 x 320 canvas 25 such tiles add up past 2^32 in the 64-bit atomics.  A tile of 255s is clipped throughout: all zeros."""
    for side in (64, 320):
        leak, src = np.full((1, side, side, 3), 254, np.uint8), np.full((1, side, side, 3), 255, np.uint8)
        want = check_sums(eng, src, leak, [af.IDENTITY])[0, 0]
        px = side * side
        assert want[0] == px and (want[7:13] == px * 254 * 254).all() and (want[13:19] == px * 255 * 255).all() and (want[19:] == px * 254 * 255).all()
    assert px * 255 * 255 > 1 << 32 and 4096 * 255 * 255 > 1 << 27
    full = np.full((2, 64, 64, 3), 255, np.uint8)
    assert not check_sums(eng, full, full, [af.IDENTITY, SHEAR]).any()
    assert not check_sums(eng, full, np.zeros_like(full), [af.IDENTITY]).any()
    one = full.copy()
    one[..., 1] = 1                                           # one channel in range is not enough
    assert not check_sums(eng, full, one, [af.IDENTITY]).any()


def test_sums_on_a_canvas_twice_the_leak(eng):
    from offmark import resync
    frames = ap.leak("svd", "A")[:2]
    canvas = (136, 200)                                   # 3 x 4 tiles over a 56 x 90 leak: tiles wholly beyond an edge leave early
    cands = [af.IDENTITY, resync.affine_of_rotation(canvas, (56, 90), 4.0), (ONE, 0, -(70 << 16), 0, ONE, -(100 << 16)), (ONE, 0, 1 << 40, 0, ONE, 0)]
    want = check_sums(eng, noise((2, *canvas, 3), 15), frames, cands)
    assert want[:, :3, 0].all() and not want[:, 3].any() and (want[:, :, 0] <= 56 * 90).all()


# ---- 2. apply colour ----------------------------------------------------------------------------------------------------------------
MATRICES = {
    "fitted": [[61136, 4523, 262, -52231], [-7209, 77594, -4719, -17236], [524, 1769, 63570, -35258]],          # 601as709's, negatives
    "identity": co.IDENTITY_MATRIX.tolist(),
    "negative": [[-ONE, 0, 0, 255 * ONE], [0, -ONE // 2, -ONE // 2, 255 * ONE], [-3 * ONE, 2 * ONE, -ONE, 128 * ONE + 32767]],
    "saturating": [[4 * ONE, 4 * ONE, 4 * ONE, 0], [-4 * ONE, -4 * ONE, -4 * ONE, 100 * ONE], [2 * ONE, -2 * ONE, 0, -32768]],
    "limits": [[co.MAX_COEFF] * 3 + [co.MAX_OFFSET], [-co.MAX_COEFF] * 3 + [-co.MAX_OFFSET], [co.MAX_COEFF, -co.MAX_COEFF, co.MAX_COEFF, -co.MAX_OFFSET]],
}


@pytest.mark.parametrize("shape", [(2, 72, 104), (1, 1, 1), (1, 2, 3), (3, 9, 13)])
def test_apply_colour_equals_the_statement(eng, shape):
    """n * h * w * 3 bytes: 44928 = 12 * 3744, then 3, 18 = 12 + 6 and 1053 = 12 * 87 + 9: every size of the tail that follows the last
    group of four pixels.  Every matrix: into a garbage buffer, in place, from an odd address, to an odd address, in place there."""
    import torch
    assert [int(np.prod(s)) * 3 % 12 for s in [(2, 72, 104), (1, 1, 1), (1, 2, 3), (3, 9, 13)]] == [0, 3, 6, 9]
    frames = noise((*shape, 3), 16)
    frames.reshape(-1, 3)[:2] = [[0, 0, 0], [255, 255, 255]][:max(1, min(2, frames.size // 3))]
    for name, m in MATRICES.items():
        m = np.asarray(m, np.int32)
        want = co.apply_colour(frames, m)
        out = torch.full((*shape, 3), 0xA5, dtype=torch.uint8, device="cuda")
        got = eng.apply_colour(cuda(frames), m, out=out)
        assert got is out and np.array_equal(got.cpu().numpy(), want), name
        dev = cuda(frames)
        assert eng.apply_colour(dev, m.astype(np.int64), out=dev) is dev and np.array_equal(dev.cpu().numpy(), want), name      # in place
        src = odd(frames)
        assert np.array_equal(eng.apply_colour(src, m).cpu().numpy(), want), name                                 # an odd source
        dst = odd(np.zeros_like(frames), 3)
        eng.apply_colour(src, m, out=dst)                                                                         # both odd
        assert np.array_equal(dst.cpu().numpy(), want), name
        assert eng.apply_colour(src, m, out=src) is src and np.array_equal(src.cpu().numpy(), want), name         # in place at an odd address
    if shape == (2, 72, 104):
        sat = co.apply_colour(frames, np.asarray(MATRICES["saturating"], np.int32))
        assert (sat == 0).any() and (sat == 255).any() and ((sat > 0) & (sat < 255)).any()
        assert np.array_equal(eng.apply_colour(cuda(frames), torch.tensor(MATRICES["fitted"])).cpu().numpy(), co.apply_colour(frames, np.asarray(MATRICES["fitted"])))
        dev = cuda(frames)
        for bad in (np.zeros((3, 3), np.int32), np.zeros((3, 4), np.float32), np.asarray(MATRICES["limits"]) + 1, np.asarray(MATRICES["limits"]) * [1, 1, 1, 2]):
            with pytest.raises(ValueError):
                eng.apply_colour(dev, bad)


def test_apply_colour_beyond_one_step_per_thread(eng):
    """2 x 4100 x 4100 pixels are 100.9 MB: more groups of 12 bytes than the 32768 workgroups of a launch have threads, so threads walk
    a second group.  Each frame alone stays below that; the two routes agree, and the first and last rows equal the statement."""
    import torch
    m = np.asarray(MATRICES["fitted"], np.int32)
    frames = torch.randint(0, 256, (2, 4100, 4100, 3), dtype=torch.uint8, device="cuda")
    assert frames.numel() // 12 > 32768 * 256 > frames[0].numel() // 12
    whole = eng.apply_colour(frames, m)
    for f in range(2):
        assert torch.equal(whole[f:f + 1], eng.apply_colour(frames[f:f + 1], m))
    for rows in (slice(0, 2), slice(4098, 4100)):
        assert np.array_equal(whole[:, rows].cpu().numpy(), co.apply_colour(frames[:, rows].cpu().numpy(), m))


# ---- 3. graph capture -----------------------------------------------------------------------------------------------------------------
def test_buffers_are_cleared_and_the_calls_are_graph_capturable(eng):
    """Calling twice into the same buffer adds nothing; the two calls capture into one HIP graph on one stream (no parallel branches)
    and replay with identical results: no allocation, no synchronisation."""
    import torch
    frames, sources = cuda(ap.leak("svd", "A")[:2]), cuda(rs.recipe_sources()[:2])
    cands = torch.from_numpy(np.asarray([registered(), ZEROS, PART], np.int64)).cuda()
    m = np.asarray(MATRICES["fitted"], np.int32)
    ref_s, ref_c = eng.colour_sums(sources, frames, cands), eng.apply_colour(frames, m)
    sums = garbage((2, 3, 28))
    for _ in range(2):
        assert eng.colour_sums(sources, frames, cands, sums=sums) is sums and torch.equal(sums, ref_s)
    assert ref_s.any() and not ref_s[:, 1].any()
    torch.cuda.synchronize()
    coloured = torch.empty_like(ref_c)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng.colour_sums(sources, frames, cands, sums=sums)    # warm-up on the capture stream
        eng.apply_colour(frames, m, out=coloured)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            eng.colour_sums(sources, frames, cands, sums=sums)
            eng.apply_colour(frames, m, out=coloured)
    sums.fill_(7)
    coloured.fill_(7)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(sums, ref_s) and torch.equal(coloured, ref_c)
    del graph
    import gc
    gc.collect()
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        eng.colour_sums(sources, frames[:1], cands)
    with pytest.raises(ValueError):
        eng.colour_sums(sources, frames, cands[:, :4])


# ---- 4. end to end on the device ------------------------------------------------------------------------------------------------------
def device_marked(eng):
    """The recipe marked ON THE DEVICE (one watermark row per segment), back on the host: u8 [12, 72, 104, 3]."""
    from offmark.generator.shuffler import Shuffler
    pay, seg = rs.recipe_payloads(), rs.recipe_segments()
    wm = np.stack([Shuffler(key=af.KEY).generate_wm(p, (af.H * af.W // 64,)) for p in pay]).astype(np.uint8)
    return eng.svd_embed(cuda(rs.recipe_sources()), wm, wm_row=cuda(seg.astype(np.int32))).cpu().numpy()


def test_colour_mapped_leaks_are_read_like_the_statement_route(eng):
    from offmark import colour
    from offmark.extract.dct_decoder import DctDecoder
    from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder
    (r0, r1), (c0, c1), _ = ap.LEAKS["A"]
    clean = af.rotate(device_marked(eng), *af.ATTACKS["2deg"])[:, r0:r1, c0:c1]
    sources = rs.recipe_sources()

    def read(decoder, frames, src):
        return colour.read_coloured_leak(decoder, frames, src, rs.recipe_segments(), CANVAS, rs.recipe_candidates(), key=af.KEY, L=af.L8,
                                         search_frames=ap.SEARCH_FRAMES)

    for name in ("601as709", "sat-0.8-gain-0.85+15"):
        leak = co.colour_map(clean, *co.ATTACKS[name])
        want = read(co.StatementDecoder(), leak, sources)
        got = read(DwtDctSvdDecoder(), cuda(leak), cuda(sources))
        c, cw = got["colour"], want["colour"]
        print(f"{name}: geometry {got['geometry']} rms {got['registration']['rms']:.3f} score {got['score']} picks "
              f"{[int(p) for p in got['picks']]} pixels {c['pixels']} residual rms {c['residual_rms']:.3f} matrix {c['matrix'].tolist()}")
        assert np.array_equal(c["lut0"], cw["lut0"]) and np.array_equal(c["matrix"], cw["matrix"]) and c["fitted"] and cw["fitted"]
        assert c["pixels"] == cw["pixels"] and c["residual_rms"] == cw["residual_rms"] and c["first_registration"] == cw["first_registration"]
        assert got["geometry"] == want["geometry"] and got["registration"] == want["registration"] and got["registration"]["converged"]
        assert list(got["picks"]) == list(want["picks"]) == list(af.CHOSEN) == [1, 0, 1] and not got["ambiguous"]
    with pytest.raises(ValueError, match="affine"):
        read(DctDecoder(alpha=20), cuda(leak), cuda(sources))
