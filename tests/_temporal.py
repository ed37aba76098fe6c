"""Shared by the clip tests (test_temporal_statement.py, test_gpu_temporal.py): the NumPy statements of the frame signature and of the
signature distances, a StatementDecoder for offmark.temporal, and the recipe.

Statement (include/offmark_hip.h: ofmk_signature_rgb8 / ofmk_signature_distances / ofmk_align_residuals_rgb8), all integers.
Y = (R + 2 G + B + 2) >> 2.  Cell (i, j), 0 <= i, j < 8, of an h x w frame covers rows (i h) >> 3 .. ((i + 1) h) >> 3 - 1 and columns
likewise in w; with A its area, sig[8 i + j] = (2 sum Y + A) // (2 A).  dist[i][t] = sum_c |a[i][c] - b[t][c]|.  The residual of leak
frame i against source library[first[i] + j] under a geometry is tests/_align.py's sums(...)[27:29] of that pair; (0, 0) where the
index leaves the library.

The recipe is a DISSOLVE, not a pan, on purpose: under a pure pan a crop offset and a time shift are the same thing, and no method can
separate them."""
import functools

import numpy as np

import offmark_oracle as orc
import _affine as af
import _align as al
import _resync as rs


def signature(frame):
    """u8 [64] of one frame u8 [h, w, 3], h, w >= 8."""
    Y = al.luma(frame)
    h, w = Y.shape
    out = np.empty(64, np.uint8)
    for i in range(8):
        for j in range(8):
            cell = Y[(i * h) >> 3:((i + 1) * h) >> 3, (j * w) >> 3:((j + 1) * w) >> 3]
            out[8 * i + j] = (2 * int(cell.sum()) + cell.size) // (2 * cell.size)
    return out


def signatures(frames):
    """u8 [n, 64]."""
    return np.stack([signature(f) for f in np.asarray(frames)])


def distances(a, b):
    """int32 [m, N]."""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    return np.abs(a[:, None, :] - b[None, :, :]).sum(axis=2).astype(np.int32)


def residuals(library, frames, first, span, geom):
    """int64 [m, span, 2]."""
    out = np.zeros((len(frames), int(span), 2), np.int64)
    for i, f in enumerate(frames):
        for j in range(int(span)):
            s = int(first[i]) + j
            if 0 <= s < len(library):
                out[i, j] = al.sums(library[s], f, geom)[27:29]
    return out


class StatementDecoder(al.StatementDecoder):
    """tests/_align.py's StatementDecoder plus the three calls offmark.temporal drives, over the statements, on host arrays."""

    def signatures_u8(self, frames):
        return signatures(frames)

    def signature_distances_u8(self, a, b):
        return distances(a, b)

    def align_residuals_u8(self, library, frames, canvas_hw, first, span, geom):
        assert tuple(library.shape[1:3]) == tuple(canvas_hw)
        return residuals(library, frames, first, span, geom)


# ---- the recipe: a 48-frame dissolve through 7 key frames of 72 x 104, six marked segments of 8 frames; the leak is frames 11..40 with
# every sixth dropped (25 frames), rotated by 2 degrees and cropped (A) or rotated by -3 degrees at step 1.10 (B) ----
H, W, T, PER, L8, KEY, COPIES = 72, 104, 48, 8, 8, 0, 2
CANVAS = (H, W)
CHOSEN = (1, 0, 1, 1, 0, 1)
KEPT = tuple(t for t in range(11, 41) if t % 6 != 4)
SEGMENTS, PICKS = [1, 2, 3, 4], [0, 1, 1, 0]
SPAN, SEARCH_FRAMES = 7, 8
LEAKS = ("A", "B")


@functools.lru_cache(maxsize=None)
def video():
    """The unmarked video: u8 [48, 72, 104, 3], read-only."""
    K = np.stack([orc.synthetic_frame(H, W, 7000 + j) for j in range(T // PER + 1)]).astype(np.int64)
    v = np.stack([((8 - t % 8) * K[t // 8] + (t % 8) * K[t // 8 + 1] + 4) // 8 for t in range(T)]).astype(np.uint8)
    v.setflags(write=False)
    return v


def payloads():
    from offmark.fingerprint import payload_for_segment
    return [payload_for_segment(s + 1, CHOSEN[s]) for s in range(T // PER)]


def candidates():
    """Keyed by absolute segment number."""
    from offmark.fingerprint import payload_for_segment
    return {s: [payload_for_segment(s + 1, c) for c in range(COPIES)] for s in range(T // PER)}


@functools.lru_cache(maxsize=None)
def oracle_marked():
    v, pay = video(), payloads()
    m = np.stack([rs.oracle_mark(v[t], pay[t // PER], KEY) for t in range(T)])
    m.setflags(write=False)
    return m


def attack(marked, which):
    """The clip cut out of the marked video and attacked: u8 [25, 56, 90, 3] (A) or [25, 72, 104, 3] (B), read-only."""
    clip = np.ascontiguousarray(np.asarray(marked)[list(KEPT)])
    if which == "A":
        out = np.ascontiguousarray(af.rotate(clip, 2.0)[:, 7:63, 5:95])
    else:
        out = np.ascontiguousarray(af.rotate(clip, -3.0, 1.10))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def leak(which):
    return attack(oracle_marked(), which)
