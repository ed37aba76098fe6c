"""GPU: the sums of a registration step and the pyramid's halving (engine.align_sums / engine.halve, DwtDctSvdDecoder.align_sums_u8 /
halve_u8, offmark.resync.read_registered_leak; build extensions, not reference semantics).

Everything is an integer, so the device is held against the NumPy statement (tests/_align.py) integer for integer, nothing masked
out; output buffers arrive filled with garbage.  End to end the real decoder and the StatementDecoder see the same bytes, hence the
same sums, and the host arithmetic between the calls is the same float64: the registered geometry is the same tuple."""
import functools

import numpy as np
import pytest

import _affine as af
import _affine_phase as ap
import _align as al
import _resync as rs

pytestmark = pytest.mark.gpu

ONE = af.ONE
CANVAS = ap.CANVAS                           # 72 x 104: 2 x 2 tiles of 64 x 64 canvas pixels, the last of each partial
ZEROS = (0, 0, 0, 0, 0, 0)                   # out of range: singular


@functools.lru_cache(maxsize=None)
def registered(which):
    """What register_leak returns for leak A or B on the statement (tests/test_align_statement.py): about 0.1 px from the truth."""
    from offmark import resync
    return resync.register_leak(al.StatementDecoder(), rs.recipe_sources()[:ap.SEARCH_FRAMES], ap.leak("svd", which)[:ap.SEARCH_FRAMES], CANVAS)["geometry"]


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


def start(leak_hw, canvas=CANVAS):
    from offmark import resync
    return resync.affine_of_rotation(canvas, leak_hw, 0.0)


def check(eng, sources, frames, cands):
    """Device sums into a garbage-filled buffer == the statement, all n * K * 29 integers."""
    n, K = len(frames), len(cands)
    buf = garbage((n, K, 29))
    got = eng.align_sums(cuda(sources), cuda(frames), np.asarray(cands, np.int64), sums=buf)
    assert got is buf and got.dtype == buf.dtype
    got, want = got.cpu().numpy(), al.statement_sums(sources, frames, cands)
    assert got.shape == want.shape == (n, K, 29)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    return want


@pytest.mark.parametrize("which", ["A", "B"])
def test_sums_equal_the_statement_on_the_recipe(eng, which):
    """Leaks of 56 x 90 and 57 x 91 under the registered geometry, the unrotated start and a flip."""
    frames, sources = ap.leak("svd", which)[:3], rs.recipe_sources()[:3]
    hw = ap.leak_hw(which)
    assert hw == {"A": (56, 90), "B": (57, 91)}[which]
    want = check(eng, sources, frames, [registered(which), start(hw), af.hflip(hw[1])])
    mse = want[:, :, 27].sum(axis=0) / want[:, :, 28].sum(axis=0)
    assert (want[:, :, 28] > 4000).all() and mse[0] < mse[1] and mse[0] < mse[2]      # the registered geometry has the smallest residual


def test_an_out_of_range_candidate_has_29_zeros(eng):
    frames, sources = ap.leak("svd", "B")[2:4], rs.recipe_sources()[2:4]
    want = check(eng, sources, frames, [start((57, 91)), ZEROS, registered("B")])              # n = 2, K = 3
    assert not want[:, 1].any() and want[:, 0].any() and want[:, 2].any()


@pytest.mark.parametrize("canvas", [(64, 64), (9, 11), (8, 8), (65, 129)])
def test_small_canvases(eng, canvas):
    """64 x 64 is exactly one tile; 9 x 11 and 8 x 8 are a fraction of one, mostly border pixels; 65 x 129 has a last tile row of one
    pixel row (a border: nothing contributes there) and a last tile column of one pixel column."""
    from offmark import resync
    frames, sources = ap.leak("svd", "B")[:2], noise((2, *canvas, 3), 7)
    cands = [af.IDENTITY, start((57, 91), canvas), resync.affine_of_rotation(canvas, (57, 91), -30.0, 0.5, (0.5, 0.25)), af.hflip(91)]
    want = check(eng, sources, frames, cands)
    assert (want[:, 0, 28] == (min(canvas[0], 57) - 2 + (canvas[0] > 57)) * (min(canvas[1], 91) - 2 + (canvas[1] > 91))).all()


def edge_candidates(K):
    """K candidates for an 8 x 8 leak on an 8 x 8 canvas: the identity with sub-pixel offsets, and around the launch-chunk edge (65535
    candidates sit in gridDim.y) four distinct small shears, two before it and two past it.  All in range, every pixel inside."""
    k = np.arange(K, dtype=np.int64)
    cands = np.stack([np.full(K, ONE), 0 * k, 3 * (k % 251), 0 * k, np.full(K, ONE), 5 * (k % 241)], axis=1)
    cands[65533:65537] = [(ONE, s, 1 << 14, -s, ONE, 1 << 14) for s in (200, 400, 600, 800)]
    return cands


def test_sums_of_candidates_past_a_launch_chunk(eng):
    """More candidates than one launch takes: rows 65533.. (two before the chunk edge, two past it) and a strided sample of the
    earlier rows equal the same candidates in a call of their own, so the second launch's candidate and output offsets (* 29) are
    right.  n = 1; the frame side of the chunk rule (launches of fewer frames once n * K workgroups pass 2^30) is not tested: it
    needs n * K >= 2^30 outputs."""
    import torch
    K, edge = 65535 + 2, 65535
    sources, frames = cuda(noise((1, 8, 8, 3), 31)), cuda(noise((1, 8, 8, 3), 32))
    cands = torch.from_numpy(edge_candidates(K)).cuda()
    full = eng.align_sums(sources, frames, cands, sums=garbage((1, K, 29)))
    assert torch.equal(full[:, edge - 2:], eng.align_sums(sources, frames, cands[edge - 2:].contiguous()))
    sample = torch.arange(0, edge - 2, 4099, device="cuda")
    assert torch.equal(full[:, sample], eng.align_sums(sources, frames, cands[sample].contiguous()))
    assert full[0, edge:, :28].any(dim=1).all() and (full[0, :, 28] == 36).all()             # 6 x 6 contributing pixels each


def test_a_canvas_twice_the_leak(eng):
    """136 x 200 canvas pixels are 3 x 4 tiles over a 57 x 91 leak: tiles wholly beyond an edge of the leak leave early, the leak's
    edges run through others."""
    from offmark import resync
    canvas = (136, 200)
    frames, sources = ap.leak("svd", "B")[:2], noise((2, *canvas, 3), 8)
    cands = [af.IDENTITY, start((57, 91), canvas), resync.affine_of_rotation(canvas, (57, 91), 4.0), (ONE, 0, -(70 << 16), 0, ONE, -(100 << 16)),
             (ONE, 0, 1 << 40, 0, ONE, 0)]
    want = check(eng, sources, frames, cands)
    assert want[:, :4, 28].all() and not want[:, 4].any() and (want[:, :, 28] <= 57 * 91).all()


@pytest.mark.parametrize("canvas", [(4096, 16), (16, 4096)])
def test_the_largest_side(eng, canvas):
    """|yc| or |xc| reaches 2048: the products are where the 64-bit accumulators are needed (a sum passes 2^40 here)."""
    H, W = canvas
    geom = (57 * ONE // H - 1, 0, 0, 0, 91 * ONE // W - 1, 0)                              # the whole canvas inside the leak
    frames, sources = ap.leak("svd", "B")[:1], noise((1, H, W, 3), 9)
    want = check(eng, sources, frames, [geom, af.IDENTITY])
    assert want[0, 0, 28] == (H - 2) * (W - 2) and np.abs(want[0, 0, :21]).max() > 1 << 40


def test_sources_and_leaks_at_odd_byte_offsets(eng):
    """Both frame stacks start 1 (sources) and 3 (leak) bytes into their buffers: no alignment is assumed."""
    import torch
    frames, sources = ap.leak("svd", "B")[:2], rs.recipe_sources()[:2]
    cands = np.asarray([registered("B"), af.hflip(91)], np.int64)
    sbuf, fbuf = torch.zeros(sources.size + 8, dtype=torch.uint8, device="cuda"), torch.zeros(frames.size + 8, dtype=torch.uint8, device="cuda")
    s, f = sbuf[1:1 + sources.size].view(sources.shape), fbuf[3:3 + frames.size].view(frames.shape)
    s.copy_(cuda(sources))
    f.copy_(cuda(frames))
    assert s.data_ptr() % 2 == 1 and f.data_ptr() % 2 == 1 and s.is_contiguous() and f.is_contiguous()
    got = eng.align_sums(s, f, cands, sums=garbage((2, 2, 29))).cpu().numpy()
    assert np.array_equal(got, al.statement_sums(sources, frames, cands))
    half = eng.halve(f).cpu().numpy()
    assert np.array_equal(half, al.halve(frames))


@pytest.mark.parametrize("hw", [(57, 91), (16, 16)])
def test_halve_equals_the_statement(eng, hw):
    import torch
    frames = noise((3, *hw, 3), 10) if hw == (16, 16) else np.array(ap.leak("svd", "B")[:3])
    out = torch.full((3, hw[0] // 2, hw[1] // 2, 3), 0xA5, dtype=torch.uint8, device="cuda")
    got = eng.halve(cuda(frames), out=out)
    assert got is out and np.array_equal(got.cpu().numpy(), al.halve(frames))
    if hw == (16, 16):
        from offmark import _hip
        with pytest.raises(_hip.HipError):
            eng.halve(got)                                                            # 8 x 8 halves to 4 x 4: refused


def test_buffers_are_cleared_and_the_call_is_graph_capturable(eng):
    """Calling twice into the same buffer adds nothing; the call captures into a HIP graph on one stream (no parallel branches) and
    replays with identical results: no allocation, no synchronisation."""
    import torch
    frames, sources = cuda(ap.leak("svd", "B")[:2]), cuda(rs.recipe_sources()[:2])
    cands = torch.from_numpy(np.asarray([registered("B"), ZEROS, af.hflip(91)], np.int64)).cuda()
    ref = eng.align_sums(sources, frames, cands)
    buf = garbage((2, 3, 29))
    for _ in range(2):
        assert eng.align_sums(sources, frames, cands, sums=buf) is buf and torch.equal(buf, ref)
    assert ref.any() and not ref[:, 1].any()
    half_ref = eng.halve(frames)
    torch.cuda.synchronize()
    half = torch.empty_like(half_ref)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng.align_sums(sources, frames, cands, sums=buf)      # warm-up on the capture stream
        eng.halve(frames, out=half)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            eng.align_sums(sources, frames, cands, sums=buf)
            eng.halve(frames, out=half)
    buf.fill_(7)
    half.fill_(7)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(buf, ref) and torch.equal(half, half_ref)
    del graph
    import gc
    gc.collect()
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        eng.align_sums(sources, frames[:1], cands)
    with pytest.raises(ValueError):
        eng.align_sums(sources, frames, cands[:, :4])


def test_a_leak_is_registered_and_read_like_the_statement_route(eng):
    from offmark import resync
    from offmark.extract.dct_decoder import DctDecoder
    from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder
    leak, sources = ap.leak("svd", "B"), rs.recipe_sources()

    def read(decoder, frames, src, **register):
        return resync.read_registered_leak(decoder, frames, src, rs.recipe_segments(), CANVAS, rs.recipe_candidates(), key=af.KEY, L=af.L8,
                                           search_frames=ap.SEARCH_FRAMES, **register)

    want = read(al.StatementDecoder(), leak, sources)
    got = read(DwtDctSvdDecoder(), cuda(leak), cuda(sources))
    print(f"geometry {got['geometry']} iterations {got['registration']['iterations']} rms {got['registration']['rms']:.3f} normalised "
          f"{got['normalised']:.4f} picks {[int(p) for p in got['picks']]}")
    assert got["geometry"] == want["geometry"] == registered("B")
    assert got["registration"] == want["registration"] and got["registration"]["converged"]
    assert list(got["picks"]) == list(af.CHOSEN) == [1, 0, 1] and got["base"] == 0 and not got["ambiguous"]
    # through the pyramid (two levels: halve on the device) from a start 17 px off
    far = resync.shift_affine(start((57, 91)), -16, 14)
    want2 = read(al.StatementDecoder(), leak, sources, start=far, levels=2)
    got2 = read(DwtDctSvdDecoder(), cuda(leak), cuda(sources), start=far, levels=2)
    assert got2["geometry"] == want2["geometry"] and got2["registration"] == want2["registration"] and len(got2["registration"]["iterations"]) == 2
    assert resync.corner_move(got2["geometry"], got["geometry"], CANVAS) <= 1 / 16 and list(got2["picks"]) == [1, 0, 1]
    with pytest.raises(ValueError, match="affine"):
        read(DctDecoder(alpha=20), cuda(leak), cuda(sources))
