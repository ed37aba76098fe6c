"""Reading a leak whose COLOURS changed: a 3 x 3 matrix plus an offset fitted against the SOURCE frames.

Build extension, not reference semantics; DwtDctSvd, blk 4, uint8 RGB.  A BT.601 / BT.709 mix-up, a saturation setting or a hue shift
is a matrix on RGB, which no per-channel curve (offmark.tone) can undo; the mark lives in U, a difference of channels, and leaves its
quantisation cell (15 wide) as soon as the channels mix: read_registered_leak and read_toned_leak then "converge" on another
subscriber.  The operator holds the source frames, so the matrix is fitted to them as the tone curve is:

  1. a histogram match of the leak against its sources (offmark.tone.lut_of_histograms) is enough to REGISTER the leak;
  2. under that geometry every canvas pixel pairs three leak bytes with three source bytes; decoder.colour_sums_u8 forms the 28 sums
     of the least-squares problem source ~ M leak + t on the device, fused with the warp, over the pixels none of whose warped leak
     bytes is clipped (0 or 255);
  3. matrix_of_sums solves the 4 x 4 normal equations exactly and rounds once to Q16; the ORIGINAL leak is mapped through the matrix
     (decoder.apply_colour_u8, integers) and read by read_registered_leak, unchanged.

The regression runs FROM the warped leak TO the source (the conditional mean, as in the tone fit): the other direction, inverted, reads
noise.  The clipped pixels must stay out of the sums: with them the fit misreads saturation and hue changes.  Host side, Python
integers and fractions, deterministic: the device and the statement (tests/_colour.py) hand the same integers in, so the same matrix
and geometries come out.

The fit costs an untouched leak about 64 % of its score (the tone fit costs 25 %), so it is a call of its own and not a default.

Not handled: a matrix FOLLOWED BY A GAMMA (the fit alone reads at a tenth of the clean score or misreads; the fit followed by
read_toned_leak rescues some cases and loses others -- there is no reliable route yet); clips (read_leak_clip / read_toned_leak_clip
under a colour matrix); a matrix that varies over the frame or over the clip; the DCT codec, 4:2:0 planes, blk 8."""
from fractions import Fraction

import numpy as np

from . import resync, tone

NSUMS = 28
ONE = 1 << 16
MAX_COEFF, MAX_OFFSET = 1 << 21, 1 << 28          # ofmk_apply_colour_rgb8's range: the sum stays inside int32
MIN_PIXELS = 384                                  # the family's floor (resync.align_step, temporal)
_PAIR = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}


def identity() -> np.ndarray:
    return np.asarray([[ONE, 0, 0, 0], [0, ONE, 0, 0], [0, 0, ONE, 0]], np.int32)


def _sums(sums28) -> list:
    a = np.asarray(resync._host(sums28))
    if a.shape != (NSUMS,) or a.dtype.kind not in "iu":
        raise ValueError(f"sums must be integers of shape [{NSUMS}]")
    return [int(v) for v in a]


def _normal_equations(s):
    """-> (G, B): G[i][j] = sum z_i z_j with z = (l0, l1, l2, 1), B[i][c] = sum z_i s_c; Python integers."""
    ll = lambda i, j: s[7 + _PAIR[(min(i, j), max(i, j))]]
    G = [[ll(i, j) for j in range(3)] + [s[1 + i]] for i in range(3)] + [[s[1], s[2], s[3], s[0]]]
    B = [[s[19 + 3 * i + c] for c in range(3)] for i in range(3)] + [[s[4], s[5], s[6]]]
    return G, B


def _solve(G, B):
    """Gauss-Jordan on fractions: the exact solution X of G X = B (4 x 4, three right sides), or None when G is singular."""
    n = len(G)
    a = [[Fraction(v) for v in G[i]] + [Fraction(v) for v in B[i]] for i in range(n)]
    for col in range(n):
        piv = next((r for r in range(col, n) if a[r][col] != 0), None)
        if piv is None:
            return None
        a[col], a[piv] = a[piv], a[col]
        p = a[col][col]
        a[col] = [v / p for v in a[col]]
        for r in range(n):
            if r != col and a[r][col] != 0:
                q = a[r][col]
                a[r] = [v - q * u for v, u in zip(a[r], a[col])]
    return [row[n:] for row in a]


def in_range(matrix) -> bool:
    """Whether int [3, 4] is a matrix ofmk_apply_colour_rgb8 takes."""
    m = np.asarray(matrix)
    return m.shape == (3, 4) and all(abs(int(m[c, j])) <= (MAX_COEFF if j < 3 else MAX_OFFSET) for c in range(3) for j in range(4))


def matrix_of_sums(sums28):
    """The least-squares matrix of decoder.colour_sums_u8's sums at one candidate, summed over frames: int64 [28] -> (int32 [3, 4],
    fitted).  The 4 x 4 normal equations of s ~ M l + t are solved exactly on fractions; entry [c][j] = round(M[c][j] * 65536),
    [c][3] = round(t[c] * 65536), Python's rounding of a Fraction (half to even).  The identity and ``fitted`` False when the count is
    below 384, the system is singular (flat content, collinear channels) or an entry leaves ofmk_apply_colour_rgb8's range."""
    s = _sums(sums28)
    if s[0] < MIN_PIXELS:
        return identity(), False
    x = _solve(*_normal_equations(s))
    if x is None:
        return identity(), False
    m = [[round(x[j][c] * ONE) for j in range(4)] for c in range(3)]
    if not in_range(m):
        return identity(), False
    return np.asarray(m, np.int32), True


def residual_rms(sums28, matrix) -> float:
    """The rms over pixels and channels of s - (M l + t), M and t the Q16 ``matrix`` as it stands (no rounding to bytes, no clipping),
    from the same sums: sum |s - m z|^2 = sum s.s - 2 m . sum z s + m^T (sum z z^T) m per channel, in exact integers; one square root.
    0.0 without pixels.  A figure to judge by, not a verdict."""
    s = _sums(sums28)
    m = np.asarray(matrix)
    if m.shape != (3, 4) or m.dtype.kind not in "iu":
        raise ValueError("matrix must be integers of shape [3, 4]")
    if s[0] <= 0:
        return 0.0
    G, B = _normal_equations(s)
    total = 0                                         # in units of 2^-32
    for c in range(3):
        mc = [int(v) for v in m[c]]
        quad = sum(mc[i] * mc[j] * G[i][j] for i in range(4) for j in range(4))
        cross = sum(mc[i] * B[i][c] for i in range(4))
        total += s[13 + _PAIR[(c, c)]] * ONE * ONE - 2 * cross * ONE + quad
    return float(np.sqrt(float(Fraction(max(total, 0), 3 * s[0] * ONE * ONE))))


def read_coloured_leak(decoder, frames, sources, segment_of_frame, canvas_hw, candidates, key=0, L: int = 8, search_frames: int = 8,
                       **register) -> dict:
    """read_registered_leak for a leak whose colours changed; the arguments are read_registered_leak's.  decoder: a DwtDctSvdDecoder
    (blk 4; anything with its histograms_u8 / apply_tone_u8 / colour_sums_u8 / apply_colour_u8 on top of what read_registered_leak
    needs -- a DctDecoder raises ValueError).  With k = ``search_frames``:
      1. lut0 = tone.lut_of_histograms of the first k leak frames and of their k sources (whole frames both), summed over frames;
      2. register_leak on apply_tone(frames[:k], lut0) against sources[:k] -> geometry g0;
      3. matrix, fitted = matrix_of_sums(colour_sums(sources[:k], frames[:k] -- the ORIGINAL leak --, [g0]) summed over frames);
      4. coloured = apply_colour(frames, matrix), all frames, then read_registered_leak(decoder, coloured, sources, ...) unchanged: it
         registers again from the default start and reads.
    -> read_registered_leak's dict plus ``colour`` = dict(lut0, matrix, fitted, pixels, residual_rms, first_registration).  Nothing is
    raised for a matrix that could not be fitted: the identity is applied and ``fitted`` says so.  No verdict: judge
    ``registration['converged']``, its ``rms`` and ``colour``."""
    canvas_hw = (int(canvas_hw[0]), int(canvas_hw[1]))
    for need in ("histograms_u8", "apply_tone_u8", "colour_sums_u8", "apply_colour_u8", "align_sums_u8", "halve_u8", "decode_soft_affine_u8"):
        if not hasattr(decoder, need):
            raise ValueError(f"{type(decoder).__name__} does not read at an affine geometry ({need}): only DwtDctSvd does")
    k = max(1, int(search_frames))
    lut0 = tone.lut_of_histograms(tone._frame_sum(decoder.histograms_u8(frames[:k])), tone._frame_sum(decoder.histograms_u8(sources[:k])))
    first = resync.register_leak(decoder, sources[:k], decoder.apply_tone_u8(frames[:k], lut0), canvas_hw, **register)
    sums = tone._frame_sum(decoder.colour_sums_u8(sources[:k], frames[:k], canvas_hw, np.asarray([first["geometry"]], dtype=np.int64)))[0]
    matrix, fitted = matrix_of_sums(sums)
    out = resync.read_registered_leak(decoder, decoder.apply_colour_u8(frames, matrix), sources, segment_of_frame, canvas_hw, candidates,
                                      key=key, L=L, search_frames=search_frames, **register)
    out["colour"] = dict(lut0=lut0, matrix=matrix, fitted=fitted, pixels=int(sums[0]), residual_rms=residual_rms(sums, matrix),
                         first_registration=first)
    return out
