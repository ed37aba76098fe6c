"""Reading a leak whose brightness, contrast or gamma changed: a per-channel tone curve fitted against the SOURCE frames.

Build extension, not reference semantics; DwtDctSvd, blk 4, uint8 RGB.  The mark is the place of a block's top singular value inside a
quantisation cell 15 wide, so a gain of a few percent moves it by more than a cell wherever U is away from 128: a screen capture, a
re-grade, a limited / full range mix-up or a player's gamma leaves offmark.resync.read_registered_leak "converged" on the wrong
subscriber.  The operator holds the source frames for the registration anyway, and they also say what every leak value was:

  1. a histogram match of the leak against its sources (no pairing of pixels) is enough to REGISTER the leak;
  2. under that geometry every canvas pixel pairs a leak value with a source value; the mean source value per leak value, made
     monotone, is the curve -- decoder.tone_sums_u8 forms the sums on the device, fused with the warp;
  3. the leak is mapped through the curve and read by read_registered_leak, unchanged.

The histogram match alone does not restore the mark (it brings the geometry to about 0.15 px and leaves the read-out at noise); the
conditional curve does.  Host side, NumPy and Python integers, deterministic: the device and the statement (tests/_tone.py) hand the
same integers in, so the same tables and geometries come out.

read_toned_leak needs sources[i] to be leak frame i's source; for a CLIP whose tone changed, offmark.temporal.read_toned_leak_clip finds
that map first (its signatures and its frame cost are tone invariant; read_leak_clip's are not) and then calls read_toned_leak.

Cross-talk between channels (hue, saturation, a BT.601 / BT.709 mix-up) is no curve: offmark.colour.read_coloured_leak fits a matrix to
the sources instead.  Not handled: a curve that varies over the clip or over the frame (vignetting), a matrix followed by a gamma, the
DCT codec, 4:2:0 planes, blk 8."""
import numpy as np

from . import resync

LEVELS = 256


def _table(a, shape, what) -> np.ndarray:
    a = np.asarray(resync._host(a))
    if a.shape != shape or a.dtype.kind not in "iu":
        raise ValueError(f"{what} must be integers of shape {list(shape)}")
    return a.astype(np.int64)


def lut_of_histograms(leak_hist, source_hist) -> np.ndarray:
    """The table that matches the leak's value distribution to the source's, per channel, in exact integers.  Both: int64 [3, 256],
    already summed over frames.  With cumulative counts Cl, Cs and totals Nl, Ns: lut[c][v] = min{s : Cs[s] * Nl >= Cl[v] * Ns} -- the
    products leave int64, so they are Python integers.  A channel without pixels on either side gets the identity.  -> uint8 [3, 256]."""
    hl, hs = _table(leak_hist, (3, LEVELS), "leak_hist"), _table(source_hist, (3, LEVELS), "source_hist")
    if (hl < 0).any() or (hs < 0).any():
        raise ValueError("histogram counts must not be negative")
    lut = np.empty((3, LEVELS), np.uint8)
    for c in range(3):
        cl, cs = np.cumsum([int(v) for v in hl[c]], dtype=object), np.cumsum([int(v) for v in hs[c]], dtype=object)
        nl, ns = int(cl[-1]), int(cs[-1])
        if nl == 0 or ns == 0:
            lut[c] = np.arange(LEVELS)
            continue
        s = 0
        for v in range(LEVELS):                       # both sides are non-decreasing in v: one walk
            want = int(cl[v]) * ns
            while int(cs[s]) * nl < want:             # ends at s <= 255: Cs[255] * Nl = Ns * Nl >= Cl[v] * Ns
                s += 1
            lut[c, v] = s
    return lut


def _isotonic(sums, counts) -> list:
    """Weighted non-decreasing isotonic fit (pool adjacent violators) of the means sums[i] / counts[i], weights counts[i] > 0.  The pools
    keep their integer sums and weights, so which neighbours violate is decided exactly; -> the fitted means, float64, one per input."""
    pools = []                                        # [sum, weight, levels]
    for s, n in zip(sums, counts):
        pools.append([int(s), int(n), 1])
        while len(pools) > 1 and pools[-2][0] * pools[-1][1] > pools[-1][0] * pools[-2][1]:      # mean before > mean after
            s1, n1, k1 = pools.pop()
            pools[-1][0] += s1
            pools[-1][1] += n1
            pools[-1][2] += k1
    out = []
    for s, n, k in pools:
        out += [s / n] * k                            # Python's int / int: the correctly rounded float64 quotient
    return out


def curve_of_sums(sums) -> np.ndarray:
    """One channel of lut_of_sums: int64 [256, 2] = (count, sum of target values) per value -> uint8 [256], non-decreasing.  Also the
    curve between two signature lists (offmark.temporal.signature_lut)."""
    t = _table(sums, (LEVELS, 2), "sums")
    if (t < 0).any():
        raise ValueError("sums must not be negative")
    have = np.flatnonzero(t[:, 0] > 0)
    if have.size < 2:
        return np.arange(LEVELS, dtype=np.uint8)
    fit = _isotonic(t[have, 1], t[have, 0])
    levels = np.arange(LEVELS, dtype=np.float64)
    return np.clip(np.rint(np.interp(levels, have.astype(np.float64), np.asarray(fit, np.float64))), 0, 255).astype(np.uint8)


def lut_of_sums(sums) -> np.ndarray:
    """The tone curve of decoder.tone_sums_u8's sums at one candidate: int64 [3, 256, 2] = (count, sum of source values) per channel
    and leak value, summed over frames.  Per channel: the levels with a count carry the mean sum / count; a weighted non-decreasing
    isotonic fit (weights = counts) goes through them; the levels without a count are filled by linear interpolation between their
    populated neighbours, constant beyond the first and the last; clip(rint(.), 0, 255).  A channel with fewer than 2 populated
    levels gets the identity.  -> uint8 [3, 256], non-decreasing per channel."""
    t = _table(sums, (3, LEVELS, 2), "sums")
    if (t < 0).any():
        raise ValueError("sums must not be negative")
    return np.stack([curve_of_sums(t[c]) for c in range(3)])


def _frame_sum(a) -> np.ndarray:
    """[n, ...] int64 on the host or the device -> [...] int64 on the host, the frames added (a frame's entries stay below 2^36)."""
    return np.asarray(resync._host(a), dtype=np.int64).sum(axis=0)


def read_toned_leak(decoder, frames, sources, segment_of_frame, canvas_hw, candidates, key=0, L: int = 8, search_frames: int = 8,
                    **register) -> dict:
    """read_registered_leak for a leak whose tone changed; the arguments are read_registered_leak's.  decoder: a DwtDctSvdDecoder
    (blk 4; anything with its histograms_u8 / tone_sums_u8 / apply_tone_u8 on top of what read_registered_leak needs -- a DctDecoder
    raises ValueError).  With k = ``search_frames``:
      1. lut0 = lut_of_histograms of the first k leak frames and of their k sources (whole frames both), summed over frames;
      2. register_leak on apply_tone(frames[:k], lut0) against sources[:k] -> geometry g0;
      3. lut = lut_of_sums(tone_sums(sources[:k], frames[:k] -- the ORIGINAL leak --, [g0]) summed over frames);
      4. toned = apply_tone(frames, lut), all frames, then read_registered_leak(decoder, toned, sources, ...) unchanged: it registers
         again from the default start and reads.
    -> read_registered_leak's dict plus ``tone`` = dict(lut0, lut, first_registration).  No verdict: judge
    ``registration['converged']`` and its ``rms``."""
    canvas_hw = (int(canvas_hw[0]), int(canvas_hw[1]))
    for need in ("histograms_u8", "tone_sums_u8", "apply_tone_u8", "align_sums_u8", "halve_u8", "decode_soft_affine_u8"):
        if not hasattr(decoder, need):
            raise ValueError(f"{type(decoder).__name__} does not read at an affine geometry ({need}): only DwtDctSvd does")
    k = max(1, int(search_frames))
    lut0 = lut_of_histograms(_frame_sum(decoder.histograms_u8(frames[:k])), _frame_sum(decoder.histograms_u8(sources[:k])))
    first = resync.register_leak(decoder, sources[:k], decoder.apply_tone_u8(frames[:k], lut0), canvas_hw, **register)
    sums = decoder.tone_sums_u8(sources[:k], frames[:k], canvas_hw, np.asarray([first["geometry"]], dtype=np.int64))
    lut = lut_of_sums(_frame_sum(sums)[0])
    out = resync.read_registered_leak(decoder, decoder.apply_tone_u8(frames, lut), sources, segment_of_frame, canvas_hw, candidates, key=key,
                                      L=L, search_frames=search_frames, **register)
    out["tone"] = dict(lut0=lut0, lut=lut, first_registration=first)
    return out
