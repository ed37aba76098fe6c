"""GPU: the tone calls (engine.histograms / tone_sums / apply_tone, DwtDctSvdDecoder.histograms_u8 / tone_sums_u8 / apply_tone_u8,
offmark.tone.read_toned_leak; build extensions, not reference semantics).

Everything is an integer, so the device is held against the NumPy statement (tests/_tone.py) exactly, nothing masked out; output
buffers arrive filled with garbage.  End to end the real decoder and the StatementDecoder see the same bytes, hence the same
histograms and sums, and the host arithmetic between the calls is the same: the tables and the geometries are the same."""
import functools

import numpy as np
import pytest

import _affine as af
import _affine_phase as ap
import _resync as rs
import _tone as tn

pytestmark = pytest.mark.gpu

ONE = af.ONE
CANVAS = ap.CANVAS                           # 72 x 104: 2 x 2 tiles of 64 x 64 canvas pixels, the last of each partial
ZEROS = (0, 0, 0, 0, 0, 0)                   # out of range: singular
PART = (ONE, 0, 30 << 16, 0, ONE, 40 << 16)  # canvas (y, x) reads leak (y + 30, x + 40): a 26 x 50 corner of the canvas is inside


@functools.lru_cache(maxsize=None)
def registered():
    """What register_leak returns for leak A on the statement: about 0.1 px from the truth."""
    from offmark import resync
    return resync.register_leak(tn.StatementDecoder(), rs.recipe_sources()[:ap.SEARCH_FRAMES], ap.leak("svd", "A")[:ap.SEARCH_FRAMES], CANVAS)["geometry"]


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


# ---- 1. histograms ------------------------------------------------------------------------------------------------------------------
def check_hist(eng, frames, dev=None):
    n = len(frames)
    buf = garbage((n, 3, 256))
    got = eng.histograms(cuda(frames) if dev is None else dev, out=buf)
    assert got is buf
    want = tn.histograms(frames)
    assert np.array_equal(got.cpu().numpy(), want), np.argwhere(got.cpu().numpy() != want)[:5]
    assert (want.sum(axis=2) == frames.shape[1] * frames.shape[2]).all()


@pytest.mark.parametrize("shape", [(3, 9, 13), (1, 1, 1), (2, 72, 104), (1, 130, 127)])
def test_histograms_equal_the_statement(eng, shape):
    """9 x 13 = 117 pixels and 1 x 1 end in a group of fewer than four pixels; 130 x 127 = 16510 pixels are two slices of a frame,
    the second a fraction, and two pixels past the last group."""
    check_hist(eng, noise((*shape, 3), 11))
    if shape == (2, 72, 104):
        check_hist(eng, np.array(rs.recipe_sources()[:2]))


def test_histograms_at_an_odd_address_and_of_flat_frames(eng):
    frames = noise((2, 57, 91, 3), 12)
    check_hist(eng, frames, odd(frames))
    flat = np.empty((2, 72, 104, 3), np.uint8)
    flat[0], flat[1] = 200, (0, 255, 7)                  # every lane of every wavefront in one bin: full contention
    check_hist(eng, flat)
    check_hist(eng, flat[:, :9, :13], odd(flat[:, :9, :13], 3))


# ---- 2. tone sums -------------------------------------------------------------------------------------------------------------------
def check_sums(eng, sources, frames, cands, dev=None):
    n, K = len(frames), len(cands)
    buf = garbage((n, K, 3, 256, 2))
    s, f = (cuda(sources), cuda(frames)) if dev is None else dev
    got = eng.tone_sums(s, f, np.asarray(cands, np.int64), sums=buf)
    assert got is buf
    got, want = got.cpu().numpy(), tn.statement_sums(sources, frames, cands)
    assert got.shape == want.shape == (n, K, 3, 256, 2)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    return want


def test_sums_equal_the_statement_on_the_recipe(eng):
    """Leak A's 56 x 90 frames on the 72 x 104 canvas, n = 3, K = 3: the registered geometry, one that covers a corner of the canvas
    only (three of the four tiles leave early or hold few pixels), one out of range."""
    frames, sources = ap.leak("svd", "A")[:3], rs.recipe_sources()[:3]
    assert ap.leak_hw("A") == (56, 90)
    want = check_sums(eng, sources, frames, [registered(), PART, ZEROS])
    inside = want[..., 0].sum(axis=3)
    assert (inside[:, 0] > 4000).all() and (inside[:, 1] == 26 * 50).all() and not want[:, 2].any()
    # the same with a tone-mapped leak: other bins
    check_sums(eng, sources, tn.tone_map(frames, 0.70, 40.0, 1.10), [registered(), PART])


def test_sums_of_flat_leaks_and_flat_sources(eng):
    """A flat leak puts every pixel of a tile into one bin per channel; a flat source gives sums = value * count."""
    frames, sources = np.array(ap.leak("svd", "A")[:2]), np.array(rs.recipe_sources()[:2])
    flat_leak = np.empty_like(frames)
    flat_leak[0], flat_leak[1] = 255, (0, 128, 3)
    want = check_sums(eng, sources, flat_leak, [registered(), PART])
    assert (np.count_nonzero(want[..., 0], axis=3) == 1).all()
    flat_src = np.empty_like(sources)
    flat_src[0], flat_src[1] = (255, 0, 9), 77
    want = check_sums(eng, flat_src, frames, [registered()])
    assert np.array_equal(want[0, 0, 0, :, 1], 255 * want[0, 0, 0, :, 0]) and not want[0, 0, 1, :, 1].any()
    check_sums(eng, flat_src, flat_leak, [registered(), ZEROS, PART])
    # a flat leak whose lanes hold different columns' runs: the left half one value, the right half another
    halves = np.empty_like(frames)
    halves[:, :, :45], halves[:, :, 45:] = 10, 240
    halves[1, 28:] = 99
    check_sums(eng, sources, halves, [registered(), af.hflip(90)])


@pytest.mark.parametrize("hw", [(72, 104), (64, 64), (9, 11), (65, 129)])
def test_the_identity_geometry_against_a_direct_count(eng, hw):
    """h = H, w = W under the identity: every canvas pixel is inside and the warped byte is the leak's, so the sums are a bincount of
    the leak weighted by the source.  64 x 64 is exactly one tile, 9 x 11 a fraction of one, 65 x 129 has a last tile row of one
    pixel row and a last tile column of one pixel column."""
    frames, sources = noise((2, *hw, 3), 13), noise((2, *hw, 3), 14)
    want = check_sums(eng, sources, frames, [af.IDENTITY])
    for f in range(2):
        for c in range(3):
            v = frames[f, :, :, c].reshape(-1)
            assert np.array_equal(want[f, 0, c, :, 0], np.bincount(v, minlength=256))
            assert np.array_equal(want[f, 0, c, :, 1], np.bincount(v, weights=sources[f, :, :, c].reshape(-1), minlength=256).astype(np.int64))


def test_sums_at_odd_addresses_and_on_a_canvas_twice_the_leak(eng):
    from offmark import resync
    frames, sources = ap.leak("svd", "A")[:2], rs.recipe_sources()[:2]
    check_sums(eng, sources, frames, [registered(), af.hflip(90)], dev=(odd(sources, 1), odd(frames, 3)))
    canvas = (136, 200)                                   # 3 x 4 tiles over a 56 x 90 leak: tiles wholly beyond an edge leave early
    cands = [af.IDENTITY, resync.affine_of_rotation(canvas, (56, 90), 4.0), (ONE, 0, -(70 << 16), 0, ONE, -(100 << 16)), (ONE, 0, 1 << 40, 0, ONE, 0)]
    want = check_sums(eng, noise((2, *canvas, 3), 15), frames, cands)
    assert want[:, :3, :, :, 0].any() and not want[:, 3].any() and (want[..., 0].sum(axis=3) <= 56 * 90).all()


def test_sums_of_candidates_past_a_launch_chunk(eng):
    """More candidates than one launch takes (65535 sit in gridDim.y): rows 65533.. (two before the chunk edge, two past it) and a
    strided sample of the earlier rows equal the same candidates in a call of their own, so the second launch's candidate and output
    offsets (* 1536) are right.  An 8 x 8 leak on an 8 x 8 canvas, n = 1: the identity with sub-pixel offsets, four distinct small
    shears around the edge; every pixel inside.  The output is 0.8 GB: one buffer, compared in slices.  The frame side of the chunk
    rule (launches of fewer frames once n * K workgroups pass 2^30) is not tested: it needs n * K >= 2^30 outputs."""
    import torch
    K, edge = 65535 + 2, 65535
    sources, frames = cuda(noise((1, 8, 8, 3), 33)), cuda(noise((1, 8, 8, 3), 34))
    k = np.arange(K, dtype=np.int64)
    cands = np.stack([np.full(K, ONE), 0 * k, 3 * (k % 251), 0 * k, np.full(K, ONE), 5 * (k % 241)], axis=1)
    cands[edge - 2:] = [(ONE, s, 1 << 14, -s, ONE, 1 << 14) for s in (200, 400, 600, 800)]
    cands = torch.from_numpy(cands).cuda()
    full = eng.tone_sums(sources, frames, cands, sums=garbage((1, K, 3, 256, 2)))
    assert torch.equal(full[:, edge - 2:], eng.tone_sums(sources, frames, cands[edge - 2:].contiguous()))
    sample = torch.arange(0, edge - 2, 4099, device="cuda")
    assert torch.equal(full[:, sample], eng.tone_sums(sources, frames, cands[sample].contiguous()))
    assert (full[0, edge:, :, :, 0].sum(dim=2) == 64).all()                    # past the edge: all 64 pixels counted in every channel


# ---- 3. apply tone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 9, 13), (1, 1, 1), (2, 72, 104), (1, 2, 2)])
def test_apply_tone_equals_the_statement(eng, shape):
    import torch
    frames, lut = noise((*shape, 3), 16), noise((3, 256), 17)
    want = tn.apply_tone(frames, lut)
    out = torch.full((*shape, 3), 0xA5, dtype=torch.uint8, device="cuda")
    got = eng.apply_tone(cuda(frames), lut, out=out)
    assert got is out and np.array_equal(got.cpu().numpy(), want)
    dev = cuda(frames)
    assert eng.apply_tone(dev, cuda(lut), out=dev) is dev and np.array_equal(dev.cpu().numpy(), want)          # in place
    src = odd(frames)
    assert np.array_equal(eng.apply_tone(src, lut).cpu().numpy(), want)                                       # an odd source
    dst = odd(np.zeros_like(frames), 3)
    eng.apply_tone(src, lut, out=dst)                                                                         # both odd
    assert np.array_equal(dst.cpu().numpy(), want)
    assert eng.apply_tone(src, lut, out=src) is src and np.array_equal(src.cpu().numpy(), want)               # in place at an odd address
    with pytest.raises(ValueError):
        eng.apply_tone(dev, lut[:2])


# ---- 4. graph capture -----------------------------------------------------------------------------------------------------------------
def test_buffers_are_cleared_and_the_calls_are_graph_capturable(eng):
    """Calling twice into the same buffers adds nothing; the three calls capture into one HIP graph on one stream (no parallel
    branches) and replay with identical results: no allocation, no synchronisation."""
    import torch
    frames, sources = cuda(ap.leak("svd", "A")[:2]), cuda(rs.recipe_sources()[:2])
    cands = torch.from_numpy(np.asarray([registered(), ZEROS, PART], np.int64)).cuda()
    lut = cuda(noise((3, 256), 18))
    ref_h, ref_s, ref_t = eng.histograms(frames), eng.tone_sums(sources, frames, cands), eng.apply_tone(frames, lut)
    hist, sums = garbage((2, 3, 256)), garbage((2, 3, 3, 256, 2))
    for _ in range(2):
        assert eng.histograms(frames, out=hist) is hist and torch.equal(hist, ref_h)
        assert eng.tone_sums(sources, frames, cands, sums=sums) is sums and torch.equal(sums, ref_s)
    assert ref_s.any() and not ref_s[:, 1].any()
    torch.cuda.synchronize()
    toned = torch.empty_like(ref_t)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng.histograms(frames, out=hist)                      # warm-up on the capture stream
        eng.tone_sums(sources, frames, cands, sums=sums)
        eng.apply_tone(frames, lut, out=toned)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            eng.histograms(frames, out=hist)
            eng.tone_sums(sources, frames, cands, sums=sums)
            eng.apply_tone(frames, lut, out=toned)
    hist.fill_(7)
    sums.fill_(7)
    toned.fill_(7)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(hist, ref_h) and torch.equal(sums, ref_s) and torch.equal(toned, ref_t)
    del graph
    import gc
    gc.collect()
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        eng.tone_sums(sources, frames[:1], cands)
    with pytest.raises(ValueError):
        eng.tone_sums(sources, frames, cands[:, :4])


# ---- 5. end to end on the device ------------------------------------------------------------------------------------------------------
def device_marked(eng):
    """The recipe marked ON THE DEVICE (one watermark row per segment), back on the host: u8 [12, 72, 104, 3]."""
    from offmark.generator.shuffler import Shuffler
    pay, seg = rs.recipe_payloads(), rs.recipe_segments()
    wm = np.stack([Shuffler(key=af.KEY).generate_wm(p, (af.H * af.W // 64,)) for p in pay]).astype(np.uint8)
    return eng.svd_embed(cuda(rs.recipe_sources()), wm, wm_row=cuda(seg.astype(np.int32))).cpu().numpy()


def test_tone_mapped_leaks_are_read_like_the_statement_route(eng):
    from offmark import tone
    from offmark.extract.dct_decoder import DctDecoder
    from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder
    (r0, r1), (c0, c1), _ = ap.LEAKS["A"]
    clean = af.rotate(device_marked(eng), *af.ATTACKS["2deg"])[:, r0:r1, c0:c1]
    sources = rs.recipe_sources()

    def read(decoder, frames, src):
        return tone.read_toned_leak(decoder, frames, src, rs.recipe_segments(), CANVAS, rs.recipe_candidates(), key=af.KEY, L=af.L8,
                                    search_frames=ap.SEARCH_FRAMES)

    for a, b, gamma in ((0.85, 15.0, 1.0), (1.0, 0.0, 0.85)):
        leak = tn.tone_map(clean, a, b, gamma)
        want = read(tn.StatementDecoder(), leak, sources)
        got = read(DwtDctSvdDecoder(), cuda(leak), cuda(sources))
        print(f"({a}, {b}, {gamma}): geometry {got['geometry']} rms {got['registration']['rms']:.3f} score {got['score']} picks "
              f"{[int(p) for p in got['picks']]}")
        assert np.array_equal(got["tone"]["lut0"], want["tone"]["lut0"]) and np.array_equal(got["tone"]["lut"], want["tone"]["lut"])
        assert got["tone"]["first_registration"] == want["tone"]["first_registration"]
        assert got["geometry"] == want["geometry"] and got["registration"] == want["registration"] and got["registration"]["converged"]
        assert list(got["picks"]) == list(want["picks"]) == list(af.CHOSEN) == [1, 0, 1] and not got["ambiguous"]
    with pytest.raises(ValueError, match="affine"):
        read(DctDecoder(alpha=20), cuda(leak), cuda(sources))
