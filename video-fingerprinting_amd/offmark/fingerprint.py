"""A/B-segment fingerprint bookkeeping on top of the per-frame payloads (host-side, integers only).

Restates the payload conventions of the reference's workflow scripts so that segments marked here are
read by its detector and vice versa:
  * segment payload, 8 bits of the segment number  -- tests/segment_mark_detect_hls.py:42-55
  * segment(4 bits) || copy(4 bits) payload         -- tests/mark_video_to_hls.py:27-43
  * pattern -> (segment, copy)                      -- tests/detect_watermarks.py:145-172
  * leak pattern -> one copy per segment            -- tests/generate_leak.py:59-108 (the selection rule)
  * view number -> base-C digit string              -- api/main.py:220-230
  * per-segment detection -> copy sequence          -- tests/detect_watermarks.py:345-364 (no-mapping branch)
  * segment file name -> segment number             -- tests/detect_watermarks.py:50-80
Pinned by tests/golden/fingerprint_layer.json: inputs/outputs of the reference's own functions
(tools/make_fingerprint_golden.py).
"""
from __future__ import annotations

import numpy as np


def payload_for_segment(segment_number: int, copy_index: int | None = None) -> np.ndarray:
    """8 payload bits, MSB first.  With ``copy_index``: 4 bits of segment % 16 then 4 bits of copy % 16."""
    if copy_index is None:
        text = format(segment_number % 256, "08b")
    else:
        text = format(segment_number % 16, "04b") + format(copy_index % 16, "04b")
    return np.array([int(b) for b in text])


def decode_pattern(pattern):
    """(segment_number, copy_index) from at least 8 bits, or (None, None)."""
    if pattern is None:
        return None, None
    bits = [int(b) for b in np.asarray(pattern).reshape(-1)]
    if len(bits) < 8:
        return None, None
    return int("".join(map(str, bits[:4])), 2), int("".join(map(str, bits[4:8])), 2)


def select_copies(pattern: str, num_segments: int, num_copies: int) -> list[int]:
    """Copy index used for each segment of a leak: digit i of ``pattern`` modulo the number of copies."""
    if len(pattern) < num_segments:
        raise ValueError(f"Pattern '{pattern}' is too short for {num_segments} segments")
    return [int(pattern[i]) % num_copies for i in range(num_segments)]


def view_to_copies(view_number: int, num_copies: int, num_segments: int) -> list[int]:
    """Base-``num_copies`` digits of the view number, most significant first, zero-padded to the segment count."""
    digits = []
    v = view_number
    while v > 0:
        digits.append(v % num_copies)
        v //= num_copies
    while len(digits) < num_segments:
        digits.append(0)
    digits.reverse()
    return digits


def segment_number_from_filename(filename: str):
    """Segment number of a segment file (tests/detect_watermarks.py:50-80): the first '_'-separated part of the
    basename that is all digits, else the first run of digits anywhere in the basename, else None."""
    import os
    import re
    base = os.path.basename(filename)
    for part in base.split("_"):
        if part.isdigit():
            return int(part)
    m = re.search(r"(\d+)", base)
    return int(m.group(1)) if m else None


def identify_copies(segment_votes: dict, segment_numbers=None) -> list[int | None]:
    """Copy sequence of a leaked stream from per-segment votes {segment: (pattern, frequency)}.
    A segment whose decoded segment field does not match its own number (mod 16) yields None."""
    keys = sorted(segment_votes) if segment_numbers is None else list(segment_numbers)
    out = []
    for s in keys:
        pattern, _freq = segment_votes[s]
        seg, copy = decode_pattern(pattern)
        out.append(copy if seg is not None and seg == s % 16 else None)
    return out


# ---------------------------------------------------------------------------------------------
# Marking N copies per segment, verifying them, and the reference's JSON sidecars
# (tests/mark_video_to_hls.py:330-434).  The pixel work is one batched GPU call for all copies when the encoder offers
# encode_copies_u8 (RGB frames) / encode_copies_planes_yuv420 (4:2:0 planes), else one per copy.
# ---------------------------------------------------------------------------------------------

def _reads_like(encoder, decoder) -> bool:
    """True when ``decoder`` reads exactly what the encoder's own verify reads: a DwtDctSvdDecoder with the encoder's channel-1
    scale and blk (the DwtDctSvd read-out is channel 1's, dwt_dct_svd_decoder.py:24), or a DctDecoder with a DctEncoder's alpha."""
    from .embed.dct_encoder import DctEncoder
    from .extract.dct_decoder import DctDecoder
    from .extract.dwt_dct_svd_decoder import DwtDctSvdDecoder
    if isinstance(encoder, DctEncoder):
        return isinstance(decoder, DctDecoder) and encoder.alpha == decoder.alpha
    return (isinstance(decoder, DwtDctSvdDecoder) and getattr(encoder, "blk", None) == decoder.blk
            and getattr(encoder, "_scales", [None] * 3)[1] == decoder._scales[1])


def copy_margins(soft, segment_of_frame, expected_raw_bits, units_per_frame: int) -> dict:
    """How far every segment of ONE marked copy is from flipping a payload position (build extension, from the soft read-outs).

    soft: int64 [n, L] soft sums of the copy's frames (2^14 fixed point, positive reads as 1: decode_soft_frames_u8 /
    decode_soft_planes_yuv420, or the one-pass copies calls' ``soft[c]``), tensor or array; segment_of_frame: int [n];
    expected_raw_bits: {segment: the L bits written at raw positions 0..L-1} -- the first L entries of the segment's watermark
    row, i.e. the shuffled payload before the key permutation is undone; units_per_frame: U, the units a frame reads out
    ((H/8)*(W/8) for the DCT codec and DwtDctSvd blk 4, the 16x16 tile count for blk 8).
    With T[i] the sum of soft[f][i] over the segment's frames and K[i] the number of units u < U with u mod L == i,
        margin = min over i of (2 e[i] - 1) T[i] / (16384 K[i] frames),   float64, in [-1, 1]
    (positions no unit lands on, K[i] == 0, are left out): 1 = every unit sits on its lattice point, <= 0 = some position does
    not read as written.  Returns {segment: margin}."""
    sums = soft.cpu().numpy() if hasattr(soft, "cpu") else np.asarray(soft)
    sums = sums.astype(np.int64)
    seg = np.asarray(segment_of_frame)
    L = sums.shape[1]
    pos = np.arange(L)
    K = np.where(pos < units_per_frame, (units_per_frame - pos + L - 1) // L, 0).astype(np.float64)
    out = {}
    for s, e in expected_raw_bits.items():
        rows = sums[seg == s]
        T = rows.sum(axis=0).astype(np.float64)
        sign = 2.0 * np.asarray(e, dtype=np.float64).reshape(-1)[:L] - 1.0
        used = K > 0
        out[s] = float(np.min(sign[used] * T[used] / (16384.0 * K[used] * rows.shape[0])))
    return out


def units_per_frame(decoder, height: int, width: int) -> int:
    """Units a frame reads out: 16x16 tiles for a DwtDctSvd decoder with blk 8, else 8x8 pixel blocks."""
    if getattr(decoder, "blk", 4) == 8:
        return ((height // 4 * 2) // 8) * ((width // 4 * 2) // 8)
    return (height // 8) * (width // 8)


def _mark_copies(device, n, H, W, n_bits, segment_of_frame, num_copies, key, min_frequency, one_pass, one_copy, read,
                 read_soft=None, units=0):
    """The bookkeeping mark_segment_copies and mark_segment_copies_yuv420 share: watermark table and rows of every (segment, copy),
    the marking (``one_pass(rows_dev [C, n], table_dev)`` -> (marked [C, ...], counts [C, n, 8] or None), or None when the
    encoder has no one-pass call; then ``one_copy(rows_dev [n], table_dev)`` per copy), the vote of every copy
    (``read(marked)`` -> counts where the marking left none) and the sidecar dicts.  ``read_soft`` (margins): one_pass may return
    the copies' soft sums [C, n, 8] as a third element, ``read_soft(marked)`` gives them where it does not, and the sidecars gain
    "segment_margins" (copy_margins with ``units`` units per frame)."""
    import torch
    from .degenerator.de_shuffler import DeShuffler
    from .dist.vote import vote_segments
    from .generator.shuffler import Shuffler

    seg = np.asarray(segment_of_frame)
    segments = [int(s) for s in np.unique(seg)]
    N = H * W // 64
    gen = Shuffler(key=key)
    deg = DeShuffler(key=key).set_shape((8,))
    index = {(s, c): i for i, (s, c) in enumerate((s, c) for s in segments for c in range(num_copies))}
    table = np.stack([gen.generate_wm(payload_for_segment(s, c), (N,)) for s in segments for c in range(num_copies)])
    table_dev = torch.from_numpy(table.astype(np.uint8)).to(device)
    copies, segment_payloads, failed = [], {}, []
    segment_copies = {str(s): [] for s in segments}
    rows_all = np.array([[index[(int(s), c)] for s in seg] for c in range(num_copies)], dtype=np.int32).reshape(num_copies, n)
    marked_all = counts_all = soft_all = None
    segment_margins = {}
    if one_pass is not None and 1 <= num_copies <= 16:
        marked_all, counts_all, *rest = one_pass(torch.from_numpy(rows_all).to(device), table_dev)
        soft_all = rest[0] if rest else None
    for c in range(num_copies):
        if marked_all is not None:
            marked = marked_all[c]
        else:
            marked = one_copy(torch.from_numpy(rows_all[c]).to(device), table_dev)
        counts = counts_all[c] if counts_all is not None else read(marked)
        votes = vote_segments(deg.degenerate_counts(counts.cpu().numpy(), n_bits), seg)
        copies.append(marked)
        if read_soft is not None:
            sums = soft_all[c] if soft_all is not None else read_soft(marked)
            per_segment = copy_margins(sums, seg, {s: table[index[(s, c)], :8] for s in segments}, units)
            segment_margins.update({f"{s}_{c}": per_segment[s] for s in segments})
        for s in segments:
            payload = payload_for_segment(s, c).tolist()
            name = f"marked_seg{s}_copy{c}.mp4"
            segment_payloads[f"{s}_{c}"] = payload
            segment_copies[str(s)].append({"file": name, "payload": payload, "copy_index": c})
            pattern, freq = votes[s]
            if pattern is None or pattern.tolist() != payload or freq < min_frequency:
                failed.append({"segment": name, "segment_number": s, "copy_index": c, "expected_pattern": payload,
                               "detected_pattern": None if pattern is None else pattern.tolist(), "frequency": freq})
    sidecars = {
        "segment_payloads": segment_payloads,
        "segment_copies": {"total_segments": len(segments), "copies_per_segment": num_copies,
                           "total_marked_segments": len(segments) * num_copies, "segments": segment_copies},
        "failed_segments": failed,
    }
    if read_soft is not None:
        sidecars["segment_margins"] = segment_margins
    return copies, sidecars



def mark_segment_copies(encoder, decoder, frames, segment_of_frame, num_copies: int, key=0, min_frequency: float = 0.5,
                        margins: bool = False):
    """Mark ``num_copies`` versions of every segment and verify each one.

    encoder / decoder: HIP codecs offering ``encode_frames_u8`` / ``decode_frames_u8`` (DctEncoder+DctDecoder or
    DwtDctSvdEncoder+DwtDctSvdDecoder).  frames: CUDA uint8 [n, H, W, 3]; segment_of_frame: int array [n].
    Returns (copies, sidecars): copies[c] is the marked tensor of copy c; sidecars holds the dicts the
    reference writes as segment_payloads.json / segment_copies.json / failed_segments.json, with the same
    keys.  A copy fails verification when its per-segment vote differs from its payload or the winning
    pattern covers fewer than ``min_frequency`` of the frames (mark_video_to_hls.py:381).
    An encoder offering ``encode_copies_u8`` marks all copies (up to 16) in one pass, and copies[c] are views of its result;
    a DwtDctSvdEncoder whose decoder reads with the same channel-1 scale and blk also hands over the verify's counts
    (``encode_verify_copies_u8``), and so does a DctEncoder whose DctDecoder has the same alpha (``encode_copies_u8`` with
    ``verify_len=8``): the decoder is then not called.  Copies and sidecars are the same either way.
    ``margins=True`` (build extension): the sidecars gain "segment_margins": {"<segment>_<copy>": copy_margins' value}, from the
    soft sums of the same one-pass call where the verify's counts come from it (measured 1.40x / 1.41x faster at 3 copies than that
    call followed by the soft read-out of each copy, profiles/copies_soft_rate.txt), else from ``decoder.decode_soft_frames_u8`` of
    each copy."""
    from .embed.dct_encoder import DctEncoder
    n, H, W, _ = frames.shape
    n_bits = decoder.bits_per_frame(H, W) if hasattr(decoder, "bits_per_frame") else H * W // 64      # DwtDctSvd(blk=8): H*W//256
    one_pass = None
    if hasattr(encoder, "encode_copies_u8"):
        # one pass for every copy: the frames are read and analyzed once (csrc/copies_kernels.hiph)
        def one_pass(rows_dev, table_dev):
            if hasattr(encoder, "encode_verify_copies_u8") and _reads_like(encoder, decoder):
                soft = {"soft": True} if margins else {}
                return encoder.encode_verify_copies_u8(frames, rows_dev, table_dev, 8, **soft)
            if isinstance(encoder, DctEncoder) and _reads_like(encoder, decoder):
                soft = {"soft": True} if margins else {}
                return encoder.encode_copies_u8(frames, rows_dev, table_dev, verify_len=8, **soft)
            return encoder.encode_copies_u8(frames, rows_dev, table_dev), None
    return _mark_copies(frames.device, n, H, W, n_bits, segment_of_frame, num_copies, key, min_frequency, one_pass,
                        lambda rows, table: encoder.encode_frames_u8(frames, wm_rows=rows, wm_table=table),
                        lambda marked: decoder.decode_frames_u8(marked, 8)[0],
                        (lambda marked: decoder.decode_soft_frames_u8(marked, 8)) if margins else None, units_per_frame(decoder, H, W))


def mark_segment_copies_yuv420(encoder, decoder, planes, height, width, segment_of_frame, num_copies: int, key=0,
                               min_frequency: float = 0.5, layout="i420", margins: bool = False, one_pass_verify: bool = False):
    """mark_segment_copies on 4:2:0 planes, what a video decoder hands over and an encoder takes: planes is CUDA uint8
    [n, 1.5*H*W] (``layout``: "i420" or "nv12"), the encoder / decoder offer ``encode_planes_yuv420`` /
    ``decode_planes_yuv420``.  Returns (copies, sidecars) with the same sidecar dicts; copies[c] are marked planes of the same
    layout.  An encoder offering ``encode_copies_planes_yuv420`` marks all copies (up to 16) in one pass
    (csrc/planar_copies_kernels.hiph) and copies[c] are views of one [C, n, 1.5*H*W] tensor; a DwtDctSvdEncoder whose decoder
    reads with the same channel-1 scale and blk also hands over the verify's counts
    (``encode_verify_copies_planes_yuv420``).  Otherwise one ``encode_planes_yuv420`` call per copy.  Copies and sidecars are
    the same either way.  ``margins=True``: "segment_margins" as mark_segment_copies, the soft sums from the DwtDctSvd one-pass
    call where the verify's counts come from it (1.27x at 3 copies), else from ``decoder.decode_soft_planes_yuv420`` of each copy (so for the DCT codec
    by default).
    ``one_pass_verify=True`` (opt-in; no effect for other encoders or a decoder that reads differently): with a DctEncoder and a
    DctDecoder of the same alpha the counts -- and with ``margins=True`` the soft sums -- come from the one-pass call
    (``encode_copies_planes_yuv420(..., verify_len=8[, soft=True])``, csrc/planar_copies_kernels.hiph) and the decoder is not called;
    copies and sidecars are the same.  Measured at 300 x 1080p against the default route (profiles/planar_copies_verify_rate.txt,
    C = 2 / 3 / 8): with margins 1.11 / 1.40 / 1.87x faster on I420 and 1.15 / 1.47 / 1.98x on NV12; WITHOUT margins 0.81 / 0.98 / 1.28x
    and 0.83 / 1.03 / 1.34x -- slower at 2 copies, a tie at 3, faster at 8 -- so the default stays False."""
    from .embed.dct_encoder import DctEncoder
    n = planes.shape[0]
    n_bits = decoder.bits_per_frame(height, width) if hasattr(decoder, "bits_per_frame") else height * width // 64
    one_pass = None
    if hasattr(encoder, "encode_copies_planes_yuv420"):
        def one_pass(rows_dev, table_dev):
            if hasattr(encoder, "encode_verify_copies_planes_yuv420") and _reads_like(encoder, decoder):
                soft = {"soft": True} if margins else {}
                return encoder.encode_verify_copies_planes_yuv420(planes, height, width, rows_dev, table_dev, 8, layout=layout, **soft)
            if one_pass_verify and isinstance(encoder, DctEncoder) and _reads_like(encoder, decoder):
                soft = {"soft": True} if margins else {}
                return encoder.encode_copies_planes_yuv420(planes, height, width, rows_dev, table_dev, layout=layout, verify_len=8, **soft)
            return encoder.encode_copies_planes_yuv420(planes, height, width, rows_dev, table_dev, layout=layout), None
    return _mark_copies(planes.device, n, height, width, n_bits, segment_of_frame, num_copies, key, min_frequency, one_pass,
                        lambda rows, table: encoder.encode_planes_yuv420(planes, height, width, wm_rows=rows, wm_table=table,
                                                                         layout=layout),
                        lambda marked: decoder.decode_planes_yuv420(marked, height, width, 8, layout=layout)[0],
                        (lambda marked: decoder.decode_soft_planes_yuv420(marked, height, width, 8, layout=layout)) if margins else None,
                        units_per_frame(decoder, height, width))


def write_sidecars(directory: str, sidecars: dict) -> list[str]:
    """Write segment_payloads.json, segment_copies.json and (if any) failed_segments.json; returns the paths."""
    import json
    import os
    os.makedirs(directory, exist_ok=True)
    paths = []
    for name in ("segment_payloads", "segment_copies", "failed_segments"):
        if name == "failed_segments" and not sidecars[name]:
            continue
        path = os.path.join(directory, name + ".json")
        with open(path, "w") as f:
            json.dump(sidecars[name], f, indent=2)
        paths.append(path)
    return paths


def identify_copies_with_payloads(segment_votes: dict, segment_payloads: dict, max_copies: int) -> list[dict]:
    """The mapping branch of detect_watermarks.py:329-344, with the segment decoded once instead of once
    per candidate copy: a copy matches when the segment's winning pattern equals that copy's recorded
    payload; among matches the highest frequency wins.  Returns one dict per segment with the keys of the
    reference's detection_results.json rows."""
    rows = []
    for s in sorted(segment_votes):
        pattern, freq = segment_votes[s]
        detected, best = None, 0
        for c in range(max_copies):
            expected = segment_payloads.get(f"{s}_{c}")
            if expected is None or pattern is None:
                continue
            if list(np.asarray(pattern).tolist()) == list(expected) and freq > best:
                best, detected = freq, c
        rows.append({"segment_number": int(s), "detected_copy_index": detected, "match_frequency": best,
                     "success": detected is not None})
    return rows
