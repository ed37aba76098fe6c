"""GPU: the read-out tail shared by every DwtDctSvd frame kernel (csrc/readout.hiph: svd_readout_begin / svd_readout_emit),
through each call that ends in it: svd_detect, svd_embed_detect, svd_detect_yuv420, svd_embed_detect_yuv420,
svd_embed_copies(L=...) and svd_embed_copies_yuv420(L=...), blk 4 and 8.

Payload lengths: 5 (no power of two), 8, 2048 (the last length the LDS histogram holds) and 2049 (the first on global atomics);
plain counts for all four, partial counts (OFMK_F_PARTIAL_COUNTS) for the three that allow them.
Shapes, the smallest at which the tail can go wrong: 136 x 168 x 3 frames is 357 units with blk 4 (two workgroups, the second
with 101 live threads) and 80 tiles with blk 8 (one part-filled workgroup); 272 x 328 x 2 is 340 tiles with blk 8 (two
workgroups).  Three copies, so the copies kernels reuse their histogram twice.  One channel-1 scale and scales = [5, 15, 20]:
the default and the MULTI instantiations.

All assertions are exact:
  * counts[..., i] == bits[..., i::L].sum(), computed on the host from the returned bits
  * partial counts summed over the tiles == the plain counts; payloads() of the two agree
  * the planar calls give the RGB chain's counts and bits (convert -> RGB call -> convert)
  * copy c == the single-copy call with wm_row = rows[c]
Every counts buffer comes from the caller, filled with a non-zero pattern: a partial row must be stored in full, zeros
included, and plain counts must be cleared in front of the adds.
"""
import functools

import numpy as np
import pytest

import offmark_oracle as orc

pytestmark = pytest.mark.gpu
P8 = np.array([0, 1, 1, 0, 0, 1, 0, 1])
LENGTHS = [5, 8, 2048, 2049]
HIST_MAX = 2048                       # csrc/common.hiph: kHistMax; partial counts need L <= this
CASES = [(4, 136, 168, 3), (8, 136, 168, 3), (8, 272, 328, 2)]      # blk, H, W, n
SCALES = {"default": dict(scale=15), "multi": dict(scales=[5, 15, 20])}
COPIES = 3
LAYOUTS = ["i420", "nv12"]


@pytest.fixture(scope="module")
def eng():
    import torch
    from offmark.engine import DctEngine
    torch.cuda.set_device(0)
    return DctEngine()


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def inputs(H, W, n):
    """Host inputs of a shape, made once: RGB frames, their planes per layout, a three-row watermark table."""
    rgb = np.stack([orc.synthetic_frame(H, W, 1001 + i) for i in range(n)])
    planes = {lay: np.stack([orc.pack_yuv420(*orc.rgb_to_yuv420(f), lay) for f in rgb]) for lay in LAYOUTS}
    wm = np.stack([orc.shuffle_generate(np.roll(P8, i), (1, H * W // 64), 0)[0] for i in range(3)]).astype(np.uint8)
    return rgb, planes, wm


def prefilled(shape):
    import torch
    numel = int(np.prod(shape))
    return (torch.arange(numel, dtype=torch.int32, device="cuda") % 7 + 1).reshape(shape)


def sums_of_bits(bits, L):
    """[..., L]: the number of ones among bits[..., i::L] (de_shuffler.py:17-18), on the host."""
    b = bits.cpu().numpy().astype(np.int64)
    pad = (-b.shape[-1]) % L
    b = np.concatenate([b, np.zeros(b.shape[:-1] + (pad,), np.int64)], axis=-1)
    return b.reshape(b.shape[:-1] + (-1, L)).sum(-2)


def read_out(eng, call, lead, blk, H, W, L):
    """call(counts=, partial=) -> (..., counts, bits), into caller-owned pre-filled buffers: plain, and partial where L allows.
    Checks the counts against the returned bits and the partial form against the plain one; returns the plain call's result."""
    import torch
    tiles = eng.lib.ofmk_svd_count_tiles(H, W, blk)
    n_bits = eng.svd_bits_per_frame(H, W, blk)
    buf = prefilled(lead + (L,))
    res = call(counts=buf, partial=False)
    counts, bits = res[-2], res[-1]
    assert counts is buf and bits.shape == lead + (n_bits,)
    assert np.array_equal(counts.cpu().numpy(), sums_of_bits(bits, L))
    if L <= HIST_MAX:
        pbuf = prefilled(lead + (tiles, L))
        pres = call(counts=pbuf, partial=True)
        assert pres[-2] is pbuf and torch.equal(pres[-1], bits)
        assert torch.equal(pbuf.sum(-2, dtype=torch.int32), counts)
        perm = torch.as_tensor(orc.payload_permutation(L, 0), dtype=torch.int32).cuda()
        assert torch.equal(eng.payloads(pbuf.reshape(-1, tiles, L), n_bits, perm), eng.payloads(counts.reshape(-1, L), n_bits, perm))
        if len(res) == 3:
            assert torch.equal(pres[0], res[0])
    return res


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("scales", sorted(SCALES))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "blk%d-%dx%dx%d" % c)
def test_readout_tail_through_every_call(eng, case, scales, L):
    import torch
    blk, H, W, n = case
    kw = dict(blk=blk, **SCALES[scales])
    rgb_h, planes_h, wm_h = inputs(H, W, n)
    rgb, wm = cuda(rgb_h), cuda(wm_h)
    rows = np.arange(n) % 3
    copy_rows = np.stack([(np.arange(n) + c) % 3 for c in range(COPIES)])
    geo = (blk, H, W, L)

    # RGB, single copy
    marked = eng.svd_embed(rgb, wm, wm_row=rows, **kw)
    read_out(eng, lambda **o: eng.svd_detect(marked, L, want_bits=True, **kw, **o), (n,), *geo)
    out, _, _ = read_out(eng, lambda **o: eng.svd_embed_detect(rgb, wm, L, wm_row=rows, want_bits=True, **kw, **o), (n,), *geo)
    assert torch.equal(out, marked)

    # RGB, copies: copy c is the single-copy call with rows[c]
    outs, counts, bits = read_out(eng, lambda **o: eng.svd_embed_copies(rgb, wm, copy_rows, L=L, want_bits=True, **kw, **o),
                                  (COPIES, n), *geo)
    for c in range(COPIES):
        o1, c1, b1 = eng.svd_embed_detect(rgb, wm, L, wm_row=copy_rows[c], want_bits=True, **kw)
        assert torch.equal(outs[c], o1) and torch.equal(counts[c], c1) and torch.equal(bits[c], b1), c

    for lay in LAYOUTS:
        planes = cuda(planes_h[lay])
        # the chain: planes -> RGB -> the RGB calls -> planes
        chain = eng.rgb_to_yuv420(eng.svd_embed(eng.yuv420_to_rgb(planes, H, W, lay), wm, wm_row=rows, **kw), lay)
        c_counts, c_bits = eng.svd_detect(eng.yuv420_to_rgb(chain, H, W, lay), L, want_bits=True, **kw)
        counts, bits = read_out(eng, lambda **o: eng.svd_detect_yuv420(chain, H, W, L, want_bits=True, layout=lay, **kw, **o), (n,), *geo)
        assert torch.equal(counts, c_counts) and torch.equal(bits, c_bits), lay
        out, counts, bits = read_out(eng, lambda **o: eng.svd_embed_detect_yuv420(planes, H, W, wm, L, wm_row=rows, want_bits=True,
                                                                                  layout=lay, **kw, **o), (n,), *geo)
        assert torch.equal(out, chain) and torch.equal(counts, c_counts) and torch.equal(bits, c_bits), lay
        # copies on planes
        outs, counts, bits = read_out(eng, lambda **o: eng.svd_embed_copies_yuv420(planes, H, W, wm, copy_rows, L=L, want_bits=True,
                                                                                   layout=lay, **kw, **o), (COPIES, n), *geo)
        for c in range(COPIES):
            o1, c1, b1 = eng.svd_embed_detect_yuv420(planes, H, W, wm, L, wm_row=copy_rows[c], want_bits=True, layout=lay, **kw)
            assert torch.equal(outs[c], o1) and torch.equal(counts[c], c1) and torch.equal(bits[c], b1), (lay, c)
