"""GPU: the tone, colour and moment kernels at their geometry and value edges (engine.tone_sums / colour_sums / align_moments /
histograms / apply_tone / apply_colour; build extensions, not reference semantics).

The inputs are tests/_value_edges.py's, and test_value_edges_statement.py holds on the CPU that they contain what they are named after.
These kernels take their warped pixels from the helpers test_gpu_geometry_edges.py proves (affine_box_misses, AffineWalk, affine_rgb)
and add logic of their own after the tap: tone_sums a run per lane and channel and a wavefront path taken when two lanes or more add
into one bin, colour_sums a clip predicate, align_moments an index table from six sums to LDS words, histograms a merge of equal
neighbours, apply_colour a clamp, a shift and a pack.  Here that logic meets
  1. the twelve edge-map cases with out-of-range maps between them, on noise and on bytes drawn from {0, 1, 254, 255};
  2. content built for the run and wavefront paths -- stripes, checkerboards, a staircase, lone lanes, thin leaks -- aligned with
     the lanes, moved 3 px down and rotated, and histogram frames with every pattern of equal neighbours;
  3. identities between device calls: colour sums as sums over tone bins, moments against residuals, a flipped map on a mirrored leak;
  4. every RGB triple through apply_colour in every slot of the 12-byte group, through apply_tone and the histogram.
Everything is an integer: every comparison is exact, nothing masked out, and output buffers arrive filled with garbage.
profiles/value_edges_tests.txt lists the wrong libraries (values only) this file was run against and the cases that saw each."""
import numpy as np
import pytest

import _colour as co
import _geometry_edges as ge
import _tone as tn
import _value_edges as ve
from test_gpu_colour import MATRICES

pytestmark = pytest.mark.gpu

N = ve.N


@pytest.fixture(scope="module")
def eng():
    import torch
    from offmark.engine import DctEngine
    torch.cuda.set_device(0)
    return DctEngine()


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the shared inputs are read-only


def garbage(shape, dtype=None):
    """The output buffer a call gets holds anything: the library writes or clears all of it."""
    import torch
    if dtype is torch.uint8:
        return torch.full(shape, 0xA5, dtype=torch.uint8, device="cuda")
    return torch.full(shape, 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")


def device_sums(eng, src, leak, cands):
    """(tone sums, colour sums) of the device, on the host."""
    cands = np.asarray(cands, np.int64)
    n, K = len(leak), len(cands)
    tone, colour = garbage((n, K, 3, 256, 2)), garbage((n, K, 28))
    assert eng.tone_sums(src, leak, cands, sums=tone) is tone and eng.colour_sums(src, leak, cands, sums=colour) is colour
    return tone.cpu().numpy(), colour.cpu().numpy()


def same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.int64
    assert np.array_equal(got, want), (np.argwhere(got != want)[:5], got[got != want][:5], want[got != want][:5])


# ---- 1. the edge maps against the statements ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["noise", "extreme"])
@pytest.mark.parametrize("case", ge.ALIGN_CASES)
def test_tone_and_colour_sums_equal_the_statement_on_the_edge_maps(eng, case, kind):
    leak_hw, canvas, _ = ge.ALIGN_CASES[case]
    cands, good, bad = ve.edge_cands(case)
    src, leak = cuda(ve.sources(canvas)), cuda(ve.leak(kind, leak_hw))
    tone, colour = device_sums(eng, src, leak, cands)
    same(tone, ve.edge_tone(case, kind))
    same(colour, ve.edge_colour(case, kind))
    assert not tone[:, bad].any() and not colour[:, bad].any()                 # out of range: zeros ...
    alone = device_sums(eng, src, leak, [cands[k] for k in good])
    same(alone[0], tone[:, good])                                              # ... and the neighbours do not change
    same(alone[1], colour[:, good])
    assert tone[:, good][..., 0].sum(axis=3).all()


@pytest.mark.parametrize("span", [1, 16])
@pytest.mark.parametrize("which", ve.MOMENT_MAPS, ids=lambda c: f"{c[0]}-{c[1]}")
def test_moments_equal_the_statement_and_the_residuals_on_the_edge_maps(eng, which, span):
    """A library of 12 frames; at span 16 the windows -3 .. 12 and 5 .. 20 leave it at either end.  sum l^2 + sum s^2 - 2 sum l s
    is align_residuals' sum e^2 and the count its count: an identity between two device calls."""
    case, k = which
    leak_hw, canvas, maps = ge.ALIGN_CASES[case]
    lib, first = cuda(ve.library(canvas)), np.array(ve.MOMENT_WINDOWS[span], np.int32)
    for kind in ("noise", "extreme"):
        leak, buf = cuda(ve.leak(kind, leak_hw)), garbage((N, span, 6))
        got = eng.align_moments(lib, leak, first, span, maps[k], out=buf)
        assert got is buf
        got = got.cpu().numpy()
        same(got, ve.edge_moments(case, k, kind, span))
        res = eng.align_residuals(lib, leak, first, span, maps[k], out=garbage((N, span, 2))).cpu().numpy()
        same(got[..., 3] + got[..., 4] - 2 * got[..., 5], res[..., 0])
        same(got[..., 0], res[..., 1])
        live = got[:, :, 0] > 0
        assert live.all() if span == 1 else (live[0, 3:15].all() and live[1, :7].all() and live.sum() == 19)


# ---- 2. structured content ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canvas", ve.CANVASES, ids=lambda c: f"{c[0]}x{c[1]}")
@pytest.mark.parametrize("name", ve.FAMILIES)
def test_tone_and_colour_sums_equal_the_statement_on_structured_content(eng, name, canvas):
    """Every frame of the family under the identity (a thin leak: 5 px to the right), the same 3 px down, and a 2 degree rotation."""
    frames, src, geoms = ve.family(name, canvas)
    tone, colour = device_sums(eng, cuda(src), cuda(frames), geoms)
    same(tone, ve.family_tone(name, canvas))
    same(colour, ve.family_colour(name, canvas))
    assert tone[..., 0].sum(axis=3).all()


@pytest.mark.parametrize("hw", ve.HIST_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_histograms_equal_the_statement_on_every_pattern_of_equal_neighbours(eng, hw):
    frames = ve.hist_frames(hw)
    buf = garbage((2, 3, 256))
    assert eng.histograms(cuda(frames), out=buf) is buf
    want = tn.histograms(frames)
    same(buf.cpu().numpy(), want)
    assert (want.sum(axis=2) == hw[0] * hw[1]).all()


# ---- 3. identities between device calls ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ge.ALIGN_CASES)
def test_colour_sums_are_sums_over_the_tone_bins_where_nothing_is_clipped(eng, case):
    """A leak in 1..254 warps to 1..254: colour_sums drops nothing, so with v the bin's value its count is tone_sums' count over all
    bins of a channel, sum l_c is sum v * count, and sum s_c is the bins' source sums."""
    leak_hw, canvas, _ = ge.ALIGN_CASES[case]
    cands, good, bad = ve.edge_cands(case)
    tone, colour = device_sums(eng, cuda(ve.sources(canvas)), cuda(ve.leak("in-range", leak_hw)), cands)
    v = np.arange(256, dtype=np.int64)
    for c in range(3):
        same(tone[:, :, c, :, 0].sum(axis=2), colour[:, :, 0])
        same((tone[:, :, c, :, 0] * v).sum(axis=2), colour[:, :, 1 + c])
        same(tone[:, :, c, :, 1].sum(axis=2), colour[:, :, 4 + c])
    assert colour[:, good, 0].all() and not colour[:, bad].any() and not tone[:, :, :, [0, 255]].any()


def test_a_flipped_map_has_the_sums_and_moments_of_the_mirrored_leak(eng):
    """ge.mirror_pairs: steep maps in multiples of 256 with no pixel in the leak's last-column fraction; the flipped map on the mirrored
    leak shows the same warped bytes, hence the same tone sums, colour sums and moments."""
    import torch
    pairs = ge.mirror_pairs(8)
    gs, ms = np.array([p[0] for p in pairs], np.int64), np.array([p[1] for p in pairs], np.int64)
    src, lib, first = cuda(ve.sources(ge.CANVAS)), cuda(ve.library(ge.CANVAS)), np.array([0, 9], np.int32)
    for kind in ("noise", "extreme"):
        leak = cuda(ve.leak(kind, ge.STEEP_LEAK))
        flipped = torch.flip(leak, dims=[2]).contiguous()
        a, b = device_sums(eng, src, leak, gs), device_sums(eng, src, flipped, ms)
        same(a[0], b[0])
        same(a[1], b[1])
        assert a[0][..., 0].sum(axis=3).all() and a[1][:, :, 0].all()
        for g, m in pairs:
            one = eng.align_moments(lib, leak, first, 3, g, out=garbage((N, 3, 6)))
            assert torch.equal(one, eng.align_moments(lib, flipped, first, 3, m, out=garbage((N, 3, 6)))) and bool(one.all())


# ---- 4. every RGB triple ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cube():
    """The cube on the device with the three prefix pixels in front of it: u8 [3 + 2^24, 3].  run[3 - k:] is the cube with k pixels
    prepended: triple i sits in slot (i + k) % 4 of its 12-byte group, and the last k triples in the tail past the last group."""
    import torch
    return torch.cat([cuda(np.asarray(ve.PREFIX, np.uint8)), cuda(ve.cube())])


def shifted(cube, k):
    """A fresh u8 [1, 1, 2^24 + k, 3] at the allocator's alignment."""
    return cube[3 - k:].clone().view(1, 1, -1, 3)


def same_bytes(got, want_prefix, want, k, what):
    """The device's [1, 1, k + 2^24, 3] against the k prefix pixels' statement (host) and the cube's (device)."""
    import torch
    body = got.view(-1, 3)[k:]
    if not torch.equal(body, want):
        bad = torch.nonzero((body != want).any(dim=1))[:5, 0]
        raise AssertionError((what, k, bad.tolist(), ve.cube()[bad.cpu().numpy()].tolist(), body[bad].tolist(), want[bad].tolist()))
    assert np.array_equal(got.view(-1, 3)[:k].cpu().numpy(), want_prefix[3 - k:]), (what, k)


@pytest.mark.parametrize("name", MATRICES)
def test_apply_colour_maps_every_triple_in_every_slot(eng, cube, name):
    import torch
    m = np.asarray(MATRICES[name], np.int32)
    want = cuda(co.apply_colour(ve.cube(), m))                                 # once per matrix
    want_prefix = co.apply_colour(np.asarray(ve.PREFIX, np.uint8), m)
    for k in range(4):
        src = shifted(cube, k)
        assert src.shape[2] % 4 == k
        out = garbage(tuple(src.shape), torch.uint8)
        assert eng.apply_colour(src, m, out=out) is out
        same_bytes(out, want_prefix, want, k, "out of place")
        assert torch.equal(src.view(-1, 3), cube[3 - k:])                      # the source is left alone
        assert eng.apply_colour(src, m, out=src) is src
        same_bytes(src, want_prefix, want, k, "in place")


def test_apply_tone_and_the_histogram_see_every_triple(eng, cube):
    import torch
    whole = cube[3:].view(1, *ve.CUBE_HW, 3)
    hist = eng.histograms(whole, out=garbage((1, 3, 256)))
    assert bool((hist == 65536).all())
    for name, lut in ve.tone_tables().items():
        want = cuda(tn.apply_tone(ve.cube(), lut))
        want_prefix = tn.apply_tone(np.asarray(ve.PREFIX, np.uint8), lut)
        for k in (0, 3):
            src = shifted(cube, k)
            out = garbage(tuple(src.shape), torch.uint8)
            assert eng.apply_tone(src, lut, out=out) is out
            same_bytes(out, want_prefix, want, k, name)
