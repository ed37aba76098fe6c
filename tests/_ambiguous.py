"""Shared by the sign-ambiguous-block tests (test_ambiguous_statement.py, test_gpu_ambiguous.py, test_gpu_parity.py,
test_golden_scipy.py): the three results the reference admits in a block whose C21 is float rounding noise, and the frame a
kernel must have written given the C21 it reports.

Statement.  The reference multiplies the quantised magnitude by np.sign(C21) (dct_encoder.py:33-35).  In a block with
|C21| <= C21_TOL ("ambiguous") that sign belongs to the last bits of the third-party DCT / cvtColor, so the reference admits
exactly three outcomes for coefficient [2][1]: +q, -q, and 0 (np.sign(0) == 0: the block keeps its pixels up to the colour round
trip, and a '1' bit is lost), with q = floor(|c| / 2 step) * 2 step (+ step for bit 1) as in qim_embed.  Which of them an
implementation must produce is named by the sign of ITS OWN C21 (the HIP library reports it: ofmk_debug_planes' c21_pre is the
record's C21, the float mark_delta consumes).  Everything else of such a block -- step, pattern, colour round trip, rounding --
is as determined as anywhere else, and is compared.

Coverage condition (asserted in candidates()): on every ambiguous block 2 * step > 4 * C21_TOL, so floor(|c| / 2 step) is 0 for
the oracle's C21 and for any C21 within the coefficient tolerance of it, and q is 0 (bit 0) or step (bit 1) whoever computes it."""
from collections import namedtuple

import numpy as np

import offmark_oracle as orc

C21_TOL = 1e-3
PIXEL_FRAC = 1e-5        # the project's pixel budget (test_gpu_parity.py): <= 1 LSB on <= 1e-5 of the samples, floor 1

Candidates = namedtuple("Candidates", "amb debug frames base")     # frames = (plus, minus, zero), base = the ordinary result; u8 [H, W, 3]


def budget(n, frac, floor=1):
    return max(floor, int(np.floor(n * frac)))


def block_pixels(blocks, H, W):
    """Per-block bool [rows, cols] -> per-pixel bool [H, W] (False on the fringe outside the block grid)."""
    m = np.zeros((H, W), bool)
    m[: blocks.shape[0] * 8, : blocks.shape[1] * 8] = np.kron(blocks, np.ones((8, 8), bool))
    return m


def candidates(frame, wm, alpha, promotion="legacy"):
    """-> Candidates(amb, debug, (plus, minus, zero), base) for one u8 frame: amb = oracle |c21_pre| <= C21_TOL per block, debug =
    the oracle's planes of its ordinary run, the three marked frames with np.sign forced to +1 / -1 / 0 in the ambiguous blocks,
    and base = that ordinary run's marked frame (mark_frame).  Outside the ambiguous blocks all three are base.
    One full oracle pass; only the ambiguous blocks are transformed again (every step of mark_frame is per block or per pixel,
    so a block alone computes the bits it computes inside a frame: test_ambiguous_statement.py holds this against full passes
    with DctEncoderOracle(sign_override=...))."""
    wm = np.asarray(wm)
    wm = wm[None] if wm.ndim == 1 else wm
    H, W, _ = frame.shape
    yuv = orc.bgr2yuv_f32(frame.astype(np.float32))
    u_in, y_in, v_in = yuv[:, :, 1].copy(), yuv[:, :, 0], yuv[:, :, 2]
    enc = orc.DctEncoderOracle(alpha=alpha, promotion=promotion)
    enc.read_wm(wm)
    base = np.around(np.clip(orc.yuv2bgr_f32(enc.encode(yuv)), a_min=0, a_max=255)).astype(np.uint8)     # mark_frame
    dbg = enc.debug
    amb = np.abs(dbg["c21_pre"]) <= C21_TOL
    rows, cols = amb.shape
    step = alpha * dbg["mask"]
    assert (2 * step[amb] > 4 * C21_TOL).all(), "an ambiguous block whose quantiser floor is not certainly 0: outside the statement"
    frames = [base.copy() for _ in range(3)]
    if amb.any():
        bits = wm[0][: rows * cols].reshape(rows, cols)[amb]
        ucoef = orc.dct8x8(orc.to_blocks(u_in)[amb])
        assert np.array_equal(ucoef[:, 2, 1], dbg["c21_pre"][amb])
        yb, vb = orc.to_blocks(y_in)[amb], orc.to_blocks(v_in)[amb]
        bi, bj = np.nonzero(amb)
        py = (bi * 8)[:, None, None] + np.arange(8)[None, :, None]
        px = (bj * 8)[:, None, None] + np.arange(8)[None, None, :]
        for out, s in zip(frames, (1.0, -1.0, 0.0)):
            c = ucoef.copy()
            c[:, 2, 1] = orc.qim_embed(ucoef[:, 2, 1], step[amb], bits, sign=s)
            rgb = orc.yuv2bgr_f32(np.stack([yb, orc.idct8x8(c), vb], axis=-1))
            out[py, px] = np.around(np.clip(rgb, a_min=0, a_max=255)).astype(np.uint8)
    return Candidates(amb, dbg, tuple(frames), base)


def expected_from_signs(cands, amb, signs):
    """One frame: per ambiguous block the candidate named by ``signs`` ([rows, cols]; > 0: plus, < 0: minus, == 0: zero); the
    oracle's ordinary result elsewhere (there the three candidates are that result)."""
    plus, minus, zero = cands
    signs = np.asarray(signs)
    assert signs.shape == amb.shape and not np.isnan(signs[amb]).any()
    H, W, _ = plus.shape
    out = plus.copy()
    for frame, pick in ((minus, amb & (signs < 0)), (zero, amb & (signs == 0))):
        px = block_pixels(pick, H, W)
        out[px] = frame[px]
    return out


def best_signs(marked, cands, amb):
    """For a marked frame whose own C21 is not known (a stored vector): per ambiguous block the candidate it is nearest to, as a
    sign array (NaN outside ambiguous blocks).  Nearest = fewest samples off, ties to plus, then minus; the zero candidate is
    admitted only where the block equals it sample for sample."""
    rows, cols = amb.shape
    off = []
    for c in cands:
        d = marked[: rows * 8, : cols * 8].astype(np.int16) - c[: rows * 8, : cols * 8].astype(np.int16)
        d = np.abs(d).reshape(rows, 8, cols, 8, 3).transpose(0, 2, 1, 3, 4).reshape(rows, cols, -1)
        off.append((d > 0).sum(-1) + 1000 * np.maximum(d.max(-1) - 1, 0))        # anything beyond 1 LSB loses to everything within it
    signs = np.where(off[1] < off[0], -1.0, 1.0)
    signs = np.where((off[2] == 0) & (np.minimum(off[0], off[1]) > 0), 0.0, signs)
    return np.where(amb, signs, np.nan)


def sign_counts(amb, signs):
    s = np.asarray(signs)[amb]
    return int((s > 0).sum()), int((s < 0).sum()), int((s == 0).sum())


def assert_frame(got, expected, where=None, what="", log=None, kind="pixels_ambiguous"):
    """The project's pixel budget over ``where`` (per-pixel bool; None: the whole frame): <= 1 LSB, on <= PIXEL_FRAC of the samples
    (floor 1).  ``log``: the parity log's function (test_gpu_parity._log), called with (kind, differing, compared) before the
    assertions; None: not logged.  Returns the number of samples off."""
    d = np.abs(got.astype(np.int16) - expected.astype(np.int16))
    if where is not None:
        d = d[where]
    if d.size == 0:
        return 0
    bad = int((d > 0).sum())
    if log is not None:
        log(kind, bad, d.size)
    assert d.max() <= 1, f"{what}: max pixel diff {d.max()} ({bad} of {d.size} samples differ)"
    assert bad <= budget(d.size, PIXEL_FRAC), f"{what}: {bad} of {d.size} samples differ"
    return bad


def assert_marked_by_own_sign(marked, cands, c21_pre, only_ambiguous=False, what="", log=None):
    """A HIP-marked frame against the frame the oracle states for the sign of the kernel's own C21 (``c21_pre`` from
    debug_planes): over the whole frame, or over the ambiguous blocks alone (where a stored vector covers the rest).
    Logs (``log``, as in assert_frame) the comparison and the + / - / 0 outcome counts; returns those counts."""
    signs = np.sign(np.asarray(c21_pre, dtype=np.float64))
    H, W, _ = marked.shape
    want = expected_from_signs(cands.frames, cands.amb, signs)
    n = sign_counts(cands.amb, signs)
    for name, k in zip(("plus", "minus", "zero"), n):
        if log is not None:
            log("ambiguous_sign_" + name, k, int(cands.amb.sum()))
    assert_frame(marked, want, block_pixels(cands.amb, H, W) if only_ambiguous else None, what=what, log=log)
    return n
