"""Shared by the toned-clip tests (test_toned_clip_statement.py, test_gpu_toned_clip.py): the NumPy statements of the six alignment
moments and of the rank signature, and a StatementDecoder for offmark.temporal.read_toned_leak_clip.

Statement (include/offmark_hip.h: ofmk_align_moments_rgb8 / ofmk_signature_ranks), all integers.  With l the luma of tests/_affine.py's
warp of leak frame i under the geometry, s the luma of library[first[i] + j] and the contributing pixels of tests/_align.py's sums
(interior canvas pixels inside the leak): mom[i][j] = (count, sum l, sum s, sum l^2, sum s^2, sum l s); six zeros where the index
leaves the library or the geometry is out of ofmk_affine's range.  rank[f][c] = #{c' : (sig[f][c'], c') < (sig[f][c], c)}: a
permutation of 0..63, ties broken by the index.

The recipe is tests/_temporal.py's clip sent through tests/_tone.py's tone maps."""
import functools

import numpy as np

import _affine as af
import _align as al
import _temporal as tp
import _tone as tn

MAPS = {"identity": (1.0, 0.0, 1.0), **tn.TONE_MAPS}
NAMED = ("gain-0.85+15", "gamma-0.85", "gain-0.70+40-gamma-1.10")       # one gain / offset, one gamma, the combined one


def moments(library, frames, first, span, geom):
    """int64 [m, span, 6]."""
    from offmark import resync
    out = np.zeros((len(frames), int(span), 6), np.int64)
    g = tuple(int(v) for v in geom)
    if not resync._affine_ok(g):
        return out
    H, W = library.shape[1:3]
    for i, f in enumerate(frames):
        warped, inside = af.warp(np.asarray(f), g, (H, W))
        ok = inside.copy()
        ok[[0, -1], :] = False
        ok[:, [0, -1]] = False
        l = al.luma(warped)[ok]
        for j in range(int(span)):
            t = int(first[i]) + j
            if 0 <= t < len(library):
                s = al.luma(library[t])[ok]
                out[i, j] = (l.size, l.sum(), s.sum(), (l * l).sum(), (s * s).sum(), (l * s).sum())
    return out


def ranks(sig):
    """u8 [n, 64] -> u8 [n, 64]."""
    s = np.asarray(sig).astype(np.int64)
    c = np.arange(64)
    below = (s[:, None, :] < s[:, :, None]) | ((s[:, None, :] == s[:, :, None]) & (c[None, None, :] < c[None, :, None]))
    return below.sum(axis=2).astype(np.uint8)


class StatementDecoder(tp.StatementDecoder, tn.StatementDecoder):
    """tests/_temporal.py's and tests/_tone.py's StatementDecoders joined, plus the two calls of the toned clip."""

    def signature_ranks_u8(self, sig):
        return ranks(sig)

    def align_moments_u8(self, library, frames, canvas_hw, first, span, geom):
        assert tuple(library.shape[1:3]) == tuple(canvas_hw)
        return moments(library, frames, first, span, geom)


@functools.lru_cache(maxsize=None)
def toned(which, name):
    """Leak ``which`` of tests/_temporal.py through tone map ``name``: u8, read-only."""
    return tn.tone_map(tp.leak(which), *MAPS[name])


@functools.lru_cache(maxsize=None)
def video_signatures():
    s = tp.signatures(tp.video())
    s.setflags(write=False)
    return s
