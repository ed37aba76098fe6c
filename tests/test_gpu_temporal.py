"""GPU: frame signatures, their distances and the residuals of a leak against a window of source frames (engine.signatures /
signature_distances / align_residuals, DwtDctSvdDecoder's *_u8 forms, offmark.temporal.read_leak_clip; build extensions, not reference
semantics).

Everything is an integer, so the device is held against the NumPy statements (tests/_temporal.py, tests/_align.py) byte for byte and
integer for integer, nothing masked out; output buffers arrive filled with garbage.  End to end the recipe is marked on the device, cut,
dropped and attacked on the host, and read with no frame map given."""
import functools

import numpy as np
import pytest

import _affine as af
import _temporal as tp

pytestmark = pytest.mark.gpu

ONE = af.ONE
CANVAS = tp.CANVAS                           # 72 x 104: 2 x 2 tiles of 64 x 64 canvas pixels, the last of each partial
TILE_M, TILE_N = 32, 256                     # temporal_kernels.hiph: kDistRows rows of a per LDS tile, kThreads rows of b per workgroup


@pytest.fixture(scope="module")
def eng():
    import torch
    from offmark.engine import DctEngine
    torch.cuda.set_device(0)
    return DctEngine()


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the shared references are read-only


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def registered(which):
    """The geometry of leak A or B registered on the statement against its true sources."""
    from offmark import resync
    k = tp.SEARCH_FRAMES
    return resync.register_leak(tp.StatementDecoder(), tp.video()[list(tp.KEPT[:k])], tp.leak(which)[:k], CANVAS)["geometry"]


# ---- 1. signatures --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("hw", [(8, 8), (13, 19), (61, 83), (72, 104), (16, 37), (9, 531)])
def test_signatures_equal_the_statement(eng, hw, n):
    """One pixel per cell; uneven cells; the recipe's sizes; widths that leave 0, 1 and 3 columns past the last group of four; 531
    columns: a lane walks three groups, the last pass partly idle.  Bands of 1 to 9 rows: fewer rows than wavefronts, and more."""
    import torch
    frames = noise((n, *hw, 3), 100 + hw[0]) if hw != CANVAS else np.array(tp.video()[20:20 + n])
    out = torch.full((n, 64), 0xA5, dtype=torch.uint8, device="cuda")
    got = eng.signatures(cuda(frames), out=out)
    assert got is out and np.array_equal(got.cpu().numpy(), tp.signatures(frames))


def test_signatures_from_a_base_pointer_offset_by_one_byte(eng):
    import torch
    frames = np.array(tp.leak("A")[:3])                                        # 56 x 90
    buf = torch.zeros(frames.size + 8, dtype=torch.uint8, device="cuda")
    f = buf[1:1 + frames.size].view(frames.shape)
    f.copy_(cuda(frames))
    assert f.data_ptr() % 2 == 1 and f.is_contiguous()
    assert np.array_equal(eng.signatures(f).cpu().numpy(), tp.signatures(frames))
    flat = np.full((1, 24, 40, 3), 255, np.uint8)                               # the largest sums: every cell reads 255
    assert (eng.signatures(cuda(flat)).cpu().numpy() == 255).all()


# ---- 2. distances ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mn", [(1, 1), (5, 130), (25, 48), (TILE_M - 1, TILE_N - 1), (TILE_M, TILE_N), (TILE_M + 1, TILE_N + 1),
                                (2 * TILE_M + 1, 3)])
def test_distances_equal_the_statement(eng, mn):
    import torch
    m, N = mn
    a, b = noise((m, 64), 7 * m + N), noise((N, 64), 11 * m + N)
    a[0], b[0] = 0, 255                                                         # the largest distance, 16320
    out = torch.full((m, N), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    got = eng.signature_distances(cuda(a), cuda(b), out=out)
    assert got is out and got.dtype == torch.int32
    want = tp.distances(a, b)
    assert np.array_equal(got.cpu().numpy(), want) and want[0, 0] == 16320


def test_distances_of_the_recipe_and_odd_base_pointers(eng):
    import torch
    sv, sl = tp.signatures(tp.video()), tp.signatures(tp.leak("B"))
    abuf, bbuf = torch.zeros(sl.size + 8, dtype=torch.uint8, device="cuda"), torch.zeros(sv.size + 8, dtype=torch.uint8, device="cuda")
    a, b = abuf[3:3 + sl.size].view(sl.shape), bbuf[1:1 + sv.size].view(sv.shape)
    a.copy_(cuda(sl))
    b.copy_(cuda(sv))
    got = eng.signature_distances(a, b).cpu().numpy()
    assert np.array_equal(got, tp.distances(sl, sv)) and got.argmin(axis=1).tolist() == list(tp.KEPT)
    with pytest.raises(ValueError):
        eng.signature_distances(a, b[:, :32])


# ---- 3. residuals ---------------------------------------------------------------------------------------------------------------
def gathered(eng, library, frames, first, span, geom):
    """align_sums' [27] and [28] of every gathered pair on the device; zeros where the index leaves the library."""
    import torch
    out = np.zeros((len(frames), span, 2), np.int64)
    lib, fr = cuda(library), cuda(frames)
    for j in range(span):
        idx = np.asarray(first) + j
        ok = (idx >= 0) & (idx < len(library))
        if ok.any():
            src = lib.index_select(0, torch.from_numpy(idx[ok]).cuda())
            sums = eng.align_sums(src, fr[torch.from_numpy(np.flatnonzero(ok)).cuda()].contiguous(), np.asarray([geom], np.int64))
            out[ok, j] = sums[:, 0, 27:29].cpu().numpy()
    return out


def residual_case(eng, which, frames_at, library, first, span, geom, statement=False):
    import torch
    frames = np.array(tp.leak(which)[frames_at])
    buf = torch.full((len(frames), span, 2), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    got = eng.align_residuals(cuda(library), cuda(frames), np.asarray(first, np.int32), span, geom, out=buf)
    assert got is buf
    got, want = got.cpu().numpy(), gathered(eng, library, frames, first, span, geom)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    if statement:
        assert np.array_equal(got, tp.residuals(library, frames, first, span, geom))
    return got


@pytest.mark.parametrize("span", [1, 7, 16])
@pytest.mark.parametrize("which", tp.LEAKS)
def test_residuals_equal_the_alignment_sums_of_the_gathered_pairs(eng, which, span):
    """Leak frames 0 and 9 (video frames 11 and 21) against the video's first 32 frames, windows centred on the truth: the residual is
    smallest there (what offmark.temporal.refine_frame_map relies on)."""
    library = tp.video()[:32]
    first = [11 - span // 2, 21 - span // 2]
    got = residual_case(eng, which, [0, 9], library, first, span, registered(which), statement=span == 7)
    assert (got[:, :, 1] > 4000).all() and (got[:, :, 1] == got[:, :1, 1]).all()             # the pixels do not depend on the source
    assert (got[:, :, 0] / got[:, :, 1]).argmin(axis=1).tolist() == [span // 2] * 2


def test_residual_windows_that_leave_the_library(eng):
    """N = 12; the windows -3..12 and 9..24 leave it at one end or both: (0, 0) there."""
    library = tp.video()[8:20]
    got = residual_case(eng, "B", [0, 9], library, [-3, 9], 16, registered("B"))
    assert not got[0, :3].any() and got[0, 3:15].all() and not got[0, 15:].any() and got[1, :3].all() and not got[1, 3:].any()
    far = residual_case(eng, "B", [0, 9], library, [-40, 12], 7, registered("B"))
    assert not far.any()


def test_residuals_under_a_geometry_that_covers_part_of_the_canvas(eng):
    """The identity puts leak A (56 x 90) on the top-left of the canvas; a shifted one leaves only the bottom-right tile with pixels,
    and the other three leave early; n = 1; a one-frame library."""
    library = tp.video()[10:13]
    got = residual_case(eng, "A", [0, 1], library, [0, 1], 3, af.IDENTITY, statement=True)
    assert (got[0, :, 1] == 55 * 89).all() and not got[1, 2].any()
    corner = (ONE, 0, -(50 << 16), 0, ONE, -(70 << 16))
    got = residual_case(eng, "A", [3], library[:1], [0], 2, corner, statement=True)
    assert got[0, 0, 1] == (72 - 50 - 1) * (104 - 70 - 1) and not got[0, 1].any()
    with pytest.raises(ValueError):
        eng.align_residuals(cuda(library), cuda(np.array(tp.leak("A")[:2])), np.zeros(3, np.int32), 3, af.IDENTITY)
    with pytest.raises(ValueError):
        eng.align_residuals(cuda(library), cuda(np.array(tp.leak("A")[:2])), np.zeros(2, np.int32), 17, af.IDENTITY)


def test_the_three_calls_are_graph_capturable(eng):
    """The calls capture into a HIP graph on one stream (no parallel branches) and replay with identical results: no allocation, no
    synchronisation; the residuals are cleared by every replay."""
    import torch
    library, frames = cuda(tp.video()[8:24]), cuda(np.array(tp.leak("B")[:4]))
    first = cuda(np.array([0, 1, 2, 3], np.int32))
    geom = registered("B")
    sig_ref = eng.signatures(library)
    dist_ref = eng.signature_distances(eng.signatures(frames), sig_ref)
    res_ref = eng.align_residuals(library, frames, first, 7, geom)
    torch.cuda.synchronize()
    sig, lsig = torch.empty_like(sig_ref), torch.empty((4, 64), dtype=torch.uint8, device="cuda")
    dist, res = torch.empty_like(dist_ref), torch.empty_like(res_ref)

    def calls():
        eng.signatures(library, out=sig)
        eng.signatures(frames, out=lsig)
        eng.signature_distances(lsig, sig, out=dist)
        eng.align_residuals(library, frames, first, 7, geom, out=res)

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        calls()                                               # warm-up on the capture stream
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            calls()
    for t in (sig, lsig, dist, res):
        t.fill_(7)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(sig, sig_ref) and torch.equal(dist, dist_ref) and torch.equal(res, res_ref) and res_ref.any()
    del graph
    import gc
    gc.collect()
    torch.cuda.synchronize()


# ---- 4. end to end on the device ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_marked():
    """The recipe's video marked ON THE DEVICE (one watermark row per segment), back on the host: u8 [48, 72, 104, 3]."""
    from offmark.engine import DctEngine
    from offmark.generator.shuffler import Shuffler
    wm = np.stack([Shuffler(key=tp.KEY).generate_wm(p, (tp.H * tp.W // 64,)) for p in tp.payloads()]).astype(np.uint8)
    rows = cuda((np.arange(tp.T) // tp.PER).astype(np.int32))
    return DctEngine().svd_embed(cuda(tp.video()), wm, wm_row=rows).cpu().numpy()


@pytest.mark.parametrize("which", tp.LEAKS)
def test_a_clip_marked_on_the_device_is_read_with_no_frame_map_given(eng, which):
    from offmark import temporal
    from offmark.extract.dct_decoder import DctDecoder
    from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder
    leak, library = tp.attack(device_marked(), which), tp.video()
    dec = DwtDctSvdDecoder()
    kw = dict(key=tp.KEY, L=tp.L8, search_frames=tp.SEARCH_FRAMES, span=tp.SPAN)
    got = temporal.read_leak_clip(dec, cuda(leak), cuda(library), tp.PER, CANVAS, tp.candidates(), **kw)
    print(f"leak {which}: coarse errors {(got['coarse_frame_map'] - np.array(tp.KEPT)).tolist()} rounds {got['rounds_used']} rms "
          f"{got['registration']['rms']:.3f} normalised {got['normalised']:.4f} picks {[int(p) for p in got['picks']]}")
    assert got["frame_map"].tolist() == list(tp.KEPT)
    assert got["segments"] == tp.SEGMENTS and [int(p) for p in got["picks"]] == tp.PICKS and not got["ambiguous"]
    assert got["registration"]["converged"] and np.abs(got["coarse_frame_map"] - np.array(tp.KEPT)).max() <= tp.SPAN // 2
    # the statement route sees the same bytes: the same maps and the same geometry
    want = temporal.read_leak_clip(tp.StatementDecoder(), leak, library, tp.PER, CANVAS, tp.candidates(), **kw)
    assert got["coarse_frame_map"].tolist() == want["coarse_frame_map"].tolist() and got["geometry"] == want["geometry"]
    assert got["rounds_used"] == want["rounds_used"] and np.array_equal(got["residual"], want["residual"])
    if which == "B":
        # a library window in the video's numbering, with the whole video's signatures
        sig = dec.signatures_u8(cuda(library))
        win = temporal.read_leak_clip(dec, cuda(leak), cuda(library[4:47]), tp.PER, CANVAS, tp.candidates(), signatures=sig, library_start=4, **kw)
        assert win["frame_map"].tolist() == list(tp.KEPT) and win["geometry"] == got["geometry"]
        with pytest.raises(ValueError, match=r"needs source frames 4\.\.46"):
            temporal.read_leak_clip(dec, cuda(leak), cuda(library[5:]), tp.PER, CANVAS, tp.candidates(), signatures=sig, library_start=5, **kw)
        with pytest.raises(ValueError, match="signatures_u8"):
            temporal.read_leak_clip(DctDecoder(alpha=20), cuda(leak), cuda(library), tp.PER, CANVAS, tp.candidates(), **kw)
