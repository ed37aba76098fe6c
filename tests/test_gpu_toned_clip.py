"""GPU: the six alignment moments of a leak against a window of source frames, the rank signature, and a toned clip read end to end
(engine.align_moments / signature_ranks, DwtDctSvdDecoder's *_u8 forms, offmark.temporal.read_toned_leak_clip; build extensions, not
reference semantics).

Everything is an integer, so the device is held against the NumPy statements (tests/_toned_clip.py) integer for integer and byte for
byte, nothing masked out; output buffers arrive filled with garbage.  Every moments case is also held against the device's own
align_residuals through the identity sum l^2 + sum s^2 - 2 sum l s = sum e^2.  End to end the recipe is marked on the device, cut,
dropped, attacked and tone mapped on the host, and read with no frame map given."""
import functools

import numpy as np
import pytest

import _affine as af
import _temporal as tp
import _tone as tn
import _toned_clip as tc

pytestmark = pytest.mark.gpu

ONE = af.ONE
CANVAS = tp.CANVAS                           # 72 x 104: 2 x 2 tiles of 64 x 64 canvas pixels, the last of each partial


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


# ---- 1. moments -----------------------------------------------------------------------------------------------------------------
def moment_case(eng, library, frames, first, span, geom):
    """The device against the statement and against its own align_residuals; the output buffer arrives filled."""
    import torch
    lib, fr = cuda(library), cuda(frames)
    buf = torch.full((len(frames), span, 6), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    got = eng.align_moments(lib, fr, np.asarray(first, np.int32), span, geom, out=buf)
    assert got is buf and got.dtype == torch.int64
    got, want = got.cpu().numpy(), tc.moments(np.asarray(library), np.asarray(frames), first, span, geom)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    res = eng.align_residuals(lib, fr, np.asarray(first, np.int32), span, geom).cpu().numpy()
    assert np.array_equal(got[..., 3] + got[..., 4] - 2 * got[..., 5], res[..., 0]) and np.array_equal(got[..., 0], res[..., 1])
    return got


@pytest.mark.parametrize("span", [1, 7, 16])
@pytest.mark.parametrize("which", tp.LEAKS)
def test_moments_equal_the_statement_on_the_recipe(eng, which, span):
    """Leak frames 0 and 9 (video frames 11 and 21) under gamma 0.85 against the video's first 32 frames, windows centred on the truth:
    the correlation cost is smallest there (what offmark.temporal.refine_frame_map_ncc relies on).  72 x 104: both tile edges."""
    from offmark import temporal
    frames = np.array(tc.toned(which, "gamma-0.85")[[0, 9]])
    got = moment_case(eng, tp.video()[:32], frames, [11 - span // 2, 21 - span // 2], span, registered(which))
    assert (got[:, :, 0] > 4000).all() and (got[:, :, [0, 1, 3]] == got[:, :1, [0, 1, 3]]).all()    # n, sum l, sum l^2: the leak's alone
    assert temporal.ncc_cost(got, 384).argmin(axis=1).tolist() == [span // 2] * 2


def test_moment_windows_that_leave_the_library(eng):
    """N = 12; the windows -3..12 and 9..24 leave it at one end or both: six zeros there."""
    library, frames = tp.video()[8:20], np.array(tp.leak("B")[[0, 9]])
    got = moment_case(eng, library, frames, [-3, 9], 16, registered("B"))
    assert not got[0, :3].any() and got[0, 3:15].all() and not got[0, 15:].any() and got[1, :3].all() and not got[1, 3:].any()
    assert not moment_case(eng, library, frames, [-40, 12], 7, registered("B")).any()
    assert moment_case(eng, library[:1], frames, [0, -2], 3, registered("B"))[:, :, 0].tolist() == [[got[0, 3, 0], 0, 0], [0, 0, got[0, 3, 0]]]


@pytest.mark.parametrize("canvas,leak_hw,geom", [
    ((8, 8), (8, 8), af.IDENTITY),                                              # one tile, 6 x 6 contributing pixels
    ((8, 8), (11, 9), (ONE + 900, -1500, (1 << 16) + 77, 1200, ONE - 300, 5000)),
    ((65, 64), (70, 60), (ONE - 2000, 1800, 2 << 16, -1700, ONE + 100, -(1 << 16))),   # a second tile row that is all border
    ((64, 65), (50, 80), (ONE, 2500, -(3 << 16), -2500, ONE, 4 << 16)),                # a second tile column that is all border
    ((129, 130), (90, 140), (52000, 3000, 1 << 16, -3000, 70000, 0)),                  # 3 x 3 tiles, pixels in a tile 2 columns wide
])
def test_moments_on_small_and_odd_canvases(eng, canvas, leak_hw, geom):
    library, frames = noise((3, *canvas, 3), canvas[0] + canvas[1]), noise((2, *leak_hw, 3), leak_hw[0])
    got = moment_case(eng, library, frames, [0, 1], 2, geom)
    assert got[0, 0, 0] > 0 and got[:, :, 0].max() <= (canvas[0] - 2) * (canvas[1] - 2)
    if geom == af.IDENTITY:
        assert (got[:, :, 0] == 36).all()


def test_moments_under_geometries_that_cover_part_of_the_canvas_or_none(eng):
    """The identity puts leak A (56 x 90) on the top-left of the canvas; a shifted one leaves only the bottom-right tile with pixels,
    and the other three leave early; one far away leaves every tile early: zeros, whatever the buffer held."""
    library, frames = tp.video()[10:13], np.array(tp.leak("A")[:2])
    got = moment_case(eng, library, frames, [0, 1], 3, af.IDENTITY)
    assert (got[0, :, 0] == 55 * 89).all() and not got[1, 2].any()
    corner = (ONE, 0, -(50 << 16), 0, ONE, -(70 << 16))
    got = moment_case(eng, library[:1], frames[:1], [0], 2, corner)
    assert got[0, 0, 0] == (72 - 50 - 1) * (104 - 70 - 1) and not got[0, 1].any()
    assert not moment_case(eng, library, frames, [0, 1], 3, (ONE, 0, 500 << 16, 0, ONE, 0)).any()
    assert not moment_case(eng, library, frames, [0, 1], 3, (ONE, 0, 0, 0, ONE, -(200 << 16))).any()
    flat = np.full((1, 24, 40, 3), 255, np.uint8)                               # the largest sums of a tile
    top = moment_case(eng, flat, flat, [0], 1, af.IDENTITY)[0, 0]
    assert top.tolist() == [22 * 38, 22 * 38 * 255, 22 * 38 * 255] + [22 * 38 * 255 * 255] * 3
    with pytest.raises(ValueError):
        eng.align_moments(cuda(library), cuda(frames), np.zeros(3, np.int32), 3, af.IDENTITY)
    with pytest.raises(ValueError):
        eng.align_moments(cuda(library), cuda(frames), np.zeros(2, np.int32), 17, af.IDENTITY)


def test_a_full_tile_of_the_largest_values(eng):
    """A 130 x 130 canvas of 255: the tile of rows and columns 64..127 has all its 4096 pixels contributing, sum l s = 4096 * 255^2 in
    one workgroup, the bound the 32-bit reduction is sized for."""
    flat = np.full((1, 130, 130, 3), 255, np.uint8)
    got = moment_case(eng, flat, flat, [0], 1, af.IDENTITY)[0, 0]
    assert got.tolist() == [128 * 128, 128 * 128 * 255, 128 * 128 * 255] + [128 * 128 * 255 * 255] * 3


# ---- 2. ranks -------------------------------------------------------------------------------------------------------------------
def rank_rows():
    rng = np.random.default_rng(11)
    return np.stack([np.full(64, 77), 200 - 3 * np.arange(64), rng.integers(0, 6, 64), rng.integers(0, 256, 64), tc.video_signatures()[20],
                     np.arange(64) // 2, rng.integers(254, 256, 64)]).astype(np.uint8)


@pytest.mark.parametrize("rows", [[0], [1], [2], [0, 1, 2, 3, 4], [2, 3, 4, 5, 6, 0, 1, 2, 3]])
def test_ranks_equal_the_statement(eng, rows):
    """n = 1 (all equal, strictly decreasing, seeded ties), n = 5 and n = 9: four frames per workgroup, the last one partly idle."""
    import torch
    sig = rank_rows()[rows]
    out = torch.full((len(rows), 64), 0xA5, dtype=torch.uint8, device="cuda")
    got = eng.signature_ranks(cuda(sig), out=out)
    assert got is out and got.dtype == torch.uint8
    got = got.cpu().numpy()
    assert np.array_equal(got, tc.ranks(sig))
    assert all(sorted(r.tolist()) == list(range(64)) for r in got)
    if rows == [0]:
        assert got[0].tolist() == list(range(64))
    if rows == [1]:
        assert got[0].tolist() == list(range(63, -1, -1))


def test_ranks_of_the_recipe_feed_the_distances(eng):
    sv, sl = tc.video_signatures(), tp.signatures(tc.toned("B", "gamma-1.20"))
    rv, rl = eng.signature_ranks(cuda(sv)), eng.signature_ranks(cuda(sl))
    assert np.array_equal(rv.cpu().numpy(), tc.ranks(sv)) and np.array_equal(rl.cpu().numpy(), tc.ranks(sl))
    got = eng.signature_distances(rl, rv).cpu().numpy()
    assert np.array_equal(got, tp.distances(tc.ranks(sl), tc.ranks(sv))) and got.max() <= 2048
    with pytest.raises(ValueError):
        eng.signature_ranks(cuda(sv)[:, :32])


def test_the_two_calls_are_graph_capturable(eng):
    """The calls capture into a HIP graph on one stream (no parallel branches) and replay with identical results: no allocation, no
    synchronisation; the moments are cleared by every replay."""
    import torch
    library, frames = cuda(tp.video()[8:24]), cuda(np.array(tp.leak("B")[:4]))
    first, sig = cuda(np.array([0, 1, 2, 3], np.int32)), cuda(tc.video_signatures())
    geom = registered("B")
    mom_ref, rank_ref = eng.align_moments(library, frames, first, 7, geom), eng.signature_ranks(sig)
    torch.cuda.synchronize()
    mom, rank = torch.empty_like(mom_ref), torch.empty_like(rank_ref)

    def calls():
        eng.signature_ranks(sig, out=rank)
        eng.align_moments(library, frames, first, 7, geom, out=mom)

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        calls()                                               # warm-up on the capture stream
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            calls()
    for t in (mom, rank):
        t.fill_(7)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(mom, mom_ref) and torch.equal(rank, rank_ref) and mom_ref.any()
    del graph
    import gc
    gc.collect()
    torch.cuda.synchronize()


# ---- 3. end to end on the device ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_marked():
    """The recipe's video marked ON THE DEVICE (one watermark row per segment), back on the host: u8 [48, 72, 104, 3]."""
    from offmark.engine import DctEngine
    from offmark.generator.shuffler import Shuffler
    wm = np.stack([Shuffler(key=tp.KEY).generate_wm(p, (tp.H * tp.W // 64,)) for p in tp.payloads()]).astype(np.uint8)
    rows = cuda((np.arange(tp.T) // tp.PER).astype(np.int32))
    return DctEngine().svd_embed(cuda(tp.video()), wm, wm_row=rows).cpu().numpy()


@pytest.mark.parametrize("which,name", [("A", "gain-0.70+40-gamma-1.10"), ("B", "gamma-0.85")])
def test_a_toned_clip_marked_on_the_device_is_read_with_no_frame_map_given(eng, which, name):
    from offmark import temporal
    from offmark.extract.dct_decoder import DctDecoder
    from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder
    leak, library = tn.tone_map(tp.attack(device_marked(), which), *tc.MAPS[name]), tp.video()
    dec = DwtDctSvdDecoder()
    kw = dict(key=tp.KEY, L=tp.L8, search_frames=tp.SEARCH_FRAMES, span=tp.SPAN)
    got = temporal.read_toned_leak_clip(dec, cuda(leak), cuda(library), tp.PER, CANVAS, tp.candidates(), **kw)
    print(f"leak {which} {name}: coarse errors {(got['coarse_frame_map'] - np.array(tp.KEPT)).tolist()} rounds {got['rounds_used']} rms "
          f"{got['registration']['rms']:.3f} ncc max {got['ncc'].max():.4f} picks {[int(p) for p in got['picks']]}")
    assert got["frame_map"].tolist() == list(tp.KEPT)
    assert got["segments"] == tp.SEGMENTS and [int(p) for p in got["picks"]] == tp.PICKS and not got["ambiguous"]
    assert got["registration"]["converged"] and np.abs(got["coarse_frame_map"] - np.array(tp.KEPT)).max() <= 2
    # the statement route sees the same bytes: the same maps, geometry, tables and picks
    want = temporal.read_toned_leak_clip(tc.StatementDecoder(), leak, library, tp.PER, CANVAS, tp.candidates(), **kw)
    assert got["coarse_frame_map"].tolist() == want["coarse_frame_map"].tolist() and got["frame_map"].tolist() == want["frame_map"].tolist()
    assert got["geometry"] == want["geometry"] and got["rounds_used"] == want["rounds_used"] and np.array_equal(got["ncc"], want["ncc"])
    assert np.array_equal(got["tone"]["lut0"], want["tone"]["lut0"]) and np.array_equal(got["tone"]["lut"], want["tone"]["lut"])
    assert [int(p) for p in got["picks"]] == [int(p) for p in want["picks"]]      # the soft sums go through float SVDs: not compared
    if which == "B":
        # a library window in the video's numbering, with the whole video's signatures
        sig = dec.signatures_u8(cuda(library))
        win = temporal.read_toned_leak_clip(dec, cuda(leak), cuda(library[4:47]), tp.PER, CANVAS, tp.candidates(), signatures=sig, library_start=4, **kw)
        assert win["frame_map"].tolist() == list(tp.KEPT) and win["geometry"] == got["geometry"]
        with pytest.raises(ValueError, match=r"needs source frames 4\.\.46"):
            temporal.read_toned_leak_clip(dec, cuda(leak), cuda(library[5:]), tp.PER, CANVAS, tp.candidates(), signatures=sig, library_start=5, **kw)
        with pytest.raises(ValueError, match="signatures_u8"):
            temporal.read_toned_leak_clip(DctDecoder(alpha=20), cuda(leak), cuda(library), tp.PER, CANVAS, tp.candidates(), **kw)
