"""DwtDctSvdDecoder on the MI355X.  Mirrors offmark.extract.dwt_dct_svd_decoder.DwtDctSvdDecoder
(reference src/offmark/extract/dwt_dct_svd_decoder.py:5-37): decode(yuv) -> float64 (1, H*W//4//blk**2), blk = 4 or 8.
This is the codec tests/detect.py constructs.  The read-out is channel 1's whatever ``scales`` says (the
reference returns wm_bits[1], dwt_dct_svd_decoder.py:24): zeros when scales[1] <= 0.  No CPU fallback."""
import numpy as np

from ..embed.dwt_dct_svd_encoder import _check_scales
from ..engine import DctEngine


class DwtDctSvdDecoder:
    def __init__(self, key=None, scales=[0, 15, 0], blk=4):
        self.key = key
        self.scales = scales
        self.blk = blk
        self._scales = _check_scales(scales, blk, need_a_mark=False)
        self._engine = None

    @property
    def engine(self) -> DctEngine:
        if self._engine is None:
            self._engine = DctEngine()
        return self._engine

    def decode(self, yuv):
        if yuv.dtype != np.float32 or yuv.ndim != 3 or yuv.shape[2] != 3:
            raise ValueError("decode expects a float32 (H, W, 3) YUV array")
        t = self.engine.torch
        dev = t.from_numpy(np.ascontiguousarray(yuv)).to(self.engine.device).unsqueeze(0)
        bits = self.engine.svd_decode_yuv(dev, scales=self._scales, blk=self.blk)
        self.block_num = bits.shape[1]
        return bits.cpu().numpy().astype(np.float64).reshape(1, -1)

    def bits_per_frame(self, height, width):
        """Length of decode()'s bit vector (dwt_dct_svd_decoder.py:14: row*col//4//blk**2): H*W//64 for blk = 4, H*W//256
        for blk = 8.  The degenerator's means divide by the slice lengths of a vector of THIS length."""
        return DctEngine.svd_bits_per_frame(height, width, self.blk)

    def decode_frames_u8(self, frames, payload_len, want_bits=False):
        """frames: CUDA uint8 [n, H, W, 3] -> (counts int32 [n, L] on device, bits or None)."""
        return self.engine.svd_detect(frames, payload_len, scales=self._scales, want_bits=want_bits, blk=self.blk)

    def decode_planes_yuv420(self, planes, height, width, payload_len, want_bits=False, layout="i420"):
        """planes: CUDA uint8 [n, 1.5*H*W] (I420 or NV12) -> (counts int32 [n, L] on device, bits or None)."""
        return self.engine.svd_detect_yuv420(planes, height, width, payload_len, scales=self._scales, want_bits=want_bits,
                                             blk=self.blk, layout=layout)

    # -- soft read-out (build extension, not reference semantics: engine.svd_detect_soft) ---------------------------------
    def decode_soft_frames_u8(self, frames, payload_len):
        """frames: CUDA uint8 [n, H, W, 3] -> soft sums int64 [n, L] on device (> 0 reads as 1)."""
        return self.engine.svd_detect_soft(frames, payload_len, scales=self._scales, blk=self.blk)

    # -- block-grid resync of cropped frames (build extension; blk 4 only: offmark.resync) ---------------------------------------
    def sync_scores_u8(self, frames):
        """frames: CUDA uint8 [n, H, W, 3], any H, W >= 8 -> int64 [n, 64] on device: per grid phase 8 * py + px the sum of
        |unit metric| over the phase's full 8x8 windows (engine.svd_sync_scores)."""
        return self.engine.svd_sync_scores(frames, scales=self._scales, blk=self.blk)

    def decode_soft_window_u8(self, frames, L, phase, canvas_cols, base=0):
        """The soft sums int64 [n, L] of the units at grid ``phase``, with the positions of a frame ``canvas_cols`` units wide
        (engine.svd_detect_soft_window)."""
        return self.engine.svd_detect_soft_window(frames, L, phase, canvas_cols, base=base, scales=self._scales, blk=self.blk)

    # -- rescaled leaks (build extension; blk 4 only: offmark.resync.read_rescaled_leak) ----------------------------------------
    def warp_scores_u8(self, frames, canvas_hw, cands):
        """frames: CUDA uint8 [n, h, w, 3], the leak; cands: int64 [K, 4] warp geometries -> int64 [n, K] on device: per candidate
        the sum of |unit metric| over the canvas units that fall inside the leak (engine.svd_warp_scores)."""
        return self.engine.svd_warp_scores(frames, canvas_hw, cands, scales=self._scales, blk=self.blk)

    def decode_soft_warp_u8(self, frames, canvas_hw, geom, L):
        """The soft sums int64 [n, L] of the leak warped by ``geom`` onto the canvas, with the uncropped frame's positions
        (engine.svd_detect_soft_warp)."""
        return self.engine.svd_detect_soft_warp(frames, canvas_hw, geom, L, scales=self._scales, blk=self.blk)

    # -- rotated leaks (build extension; blk 4 only: offmark.resync.read_rescaled_leak with [K, 6] geometries) --------------------
    def affine_scores_u8(self, frames, canvas_hw, cands):
        """warp_scores_u8 over affine candidates, int64 [K, 6] (engine.svd_affine_scores)."""
        return self.engine.svd_affine_scores(frames, canvas_hw, cands, scales=self._scales, blk=self.blk)

    def affine_phase_scores_u8(self, frames, canvas_hw, cands):
        """affine_scores_u8 of every candidate under all 64 whole-pixel shifts of the canvas: (scores int64 [n, K, 64], units
        int64 [K, 64]) at index 8 * py + px (engine.svd_affine_phase_scores; offmark.resync.best_shifted_geometry)."""
        return self.engine.svd_affine_phase_scores(frames, canvas_hw, cands, scales=self._scales, blk=self.blk)

    def decode_soft_affine_u8(self, frames, canvas_hw, geom, L):
        """decode_soft_warp_u8 at an affine ``geom`` of six (engine.svd_detect_soft_affine)."""
        return self.engine.svd_detect_soft_affine(frames, canvas_hw, geom, L, scales=self._scales, blk=self.blk)

    # -- leaks read against their source frames (build extension: offmark.resync.register_leak / read_registered_leak) ------------
    def align_sums_u8(self, sources, frames, canvas_hw, cands):
        """sources: CUDA uint8 [n, H, W, 3] with (H, W) = canvas_hw, frames: CUDA uint8 [n, h, w, 3], cands: int64 [K, 6] -> int64
        [n, K, 29] on device: the sums of one registration step (engine.align_sums)."""
        if tuple(int(v) for v in sources.shape[1:3]) != (int(canvas_hw[0]), int(canvas_hw[1])):
            raise ValueError("the source frames must have the canvas's size")
        return self.engine.align_sums(sources, frames, cands)

    def halve_u8(self, frames):
        """frames: CUDA uint8 [n, h, w, 3] -> CUDA uint8 [n, h // 2, w // 2, 3], the 2x2 box (engine.halve)."""
        return self.engine.halve(frames)

    # -- a leaked clip's frames matched to the source video's (build extension: offmark.temporal.read_leak_clip) ------------------------
    def signatures_u8(self, frames):
        """frames: CUDA uint8 [n, h, w, 3] -> CUDA uint8 [n, 64], the 8 x 8 luma thumbnails (engine.signatures)."""
        return self.engine.signatures(frames)

    def signature_distances_u8(self, a, b):
        """a: CUDA uint8 [m, 64], b: CUDA uint8 [N, 64] -> int32 [m, N] on device, the L1 distances (engine.signature_distances)."""
        return self.engine.signature_distances(a, b)

    def align_residuals_u8(self, library, frames, canvas_hw, first, span, geom):
        """library: CUDA uint8 [N, H, W, 3] with (H, W) = canvas_hw, frames: CUDA uint8 [m, h, w, 3], first: int32 [m] -> int64
        [m, span, 2] on device: (sum e^2, contributing pixels) of frame i against library[first[i] + j] under ``geom``
        (engine.align_residuals)."""
        if tuple(int(v) for v in library.shape[1:3]) != (int(canvas_hw[0]), int(canvas_hw[1])):
            raise ValueError("the library frames must have the canvas's size")
        return self.engine.align_residuals(library, frames, first, span, geom)

    # -- a leaked clip whose tone changed as well (build extension: offmark.temporal.read_toned_leak_clip) ------------------------------
    def signature_ranks_u8(self, sig):
        """sig: CUDA uint8 [n, 64] -> CUDA uint8 [n, 64], every signature's cells ranked 0..63, ties by index (engine.signature_ranks)."""
        return self.engine.signature_ranks(sig)

    def align_moments_u8(self, library, frames, canvas_hw, first, span, geom):
        """align_residuals_u8's arguments -> int64 [m, span, 6] on device: (count, sum l, sum s, sum l^2, sum s^2, sum l s) of frame
        i's warped luma l against the luma s of library[first[i] + j] under ``geom`` (engine.align_moments)."""
        if tuple(int(v) for v in library.shape[1:3]) != (int(canvas_hw[0]), int(canvas_hw[1])):
            raise ValueError("the library frames must have the canvas's size")
        return self.engine.align_moments(library, frames, first, span, geom)

    # -- leaks whose brightness, contrast or gamma changed (build extension: offmark.tone.read_toned_leak) -----------------------------
    def histograms_u8(self, frames):
        """frames: CUDA uint8 [n, h, w, 3] -> int64 [n, 3, 256] on device, the per-channel histograms (engine.histograms)."""
        return self.engine.histograms(frames)

    def tone_sums_u8(self, sources, frames, canvas_hw, cands):
        """sources: CUDA uint8 [n, H, W, 3] with (H, W) = canvas_hw, frames: CUDA uint8 [n, h, w, 3], cands: int64 [K, 6] -> int64
        [n, K, 3, 256, 2] on device: per leak value the count and the sum of the source's values (engine.tone_sums)."""
        if tuple(int(v) for v in sources.shape[1:3]) != (int(canvas_hw[0]), int(canvas_hw[1])):
            raise ValueError("the source frames must have the canvas's size")
        return self.engine.tone_sums(sources, frames, cands)

    def apply_tone_u8(self, frames, lut):
        """frames: CUDA uint8 [n, h, w, 3], lut: uint8 [3, 256] -> CUDA uint8 [n, h, w, 3], lut[c][value] per channel
        (engine.apply_tone)."""
        return self.engine.apply_tone(frames, lut)

    # -- leaks whose colours changed: a BT.601 / 709 mix-up, saturation, hue (build extension: offmark.colour.read_coloured_leak) ------
    def colour_sums_u8(self, sources, frames, canvas_hw, cands):
        """sources: CUDA uint8 [n, H, W, 3] with (H, W) = canvas_hw, frames: CUDA uint8 [n, h, w, 3], cands: int64 [K, 6] -> int64
        [n, K, 28] on device: the least-squares sums of source ~ M leak + t over the unclipped pixels (engine.colour_sums)."""
        if tuple(int(v) for v in sources.shape[1:3]) != (int(canvas_hw[0]), int(canvas_hw[1])):
            raise ValueError("the source frames must have the canvas's size")
        return self.engine.colour_sums(sources, frames, cands)

    def apply_colour_u8(self, frames, matrix):
        """frames: CUDA uint8 [n, h, w, 3], matrix: host int32 [3, 4] in Q16 -> CUDA uint8 [n, h, w, 3], the matrix and offset applied to
        every pixel in integers (engine.apply_colour)."""
        return self.engine.apply_colour(frames, matrix)

    def sync_scores_planes_yuv420(self, planes, height, width, layout="i420"):
        """planes: CUDA uint8 [n, 1.5*H*W] (I420 or NV12), even H, W >= 8 -> int64 [n, 64] on device: sync_scores_u8's sums at the
        phases with even py and px, 0 elsewhere -- an odd crop offset does not exist on 4:2:0 planes (engine.svd_sync_scores_yuv420)."""
        return self.engine.svd_sync_scores_yuv420(planes, height, width, scales=self._scales, blk=self.blk, layout=layout)

    def decode_soft_window_planes_yuv420(self, planes, height, width, L, phase, canvas_cols, base=0, layout="i420"):
        """The soft sums int64 [n, L] of the units at the even grid ``phase``, with the positions of a frame ``canvas_cols`` units
        wide (engine.svd_detect_soft_window_yuv420)."""
        return self.engine.svd_detect_soft_window_yuv420(planes, height, width, L, phase, canvas_cols, base=base, scales=self._scales,
                                                         blk=self.blk, layout=layout)

    def decode_soft_planes_yuv420(self, planes, height, width, payload_len, layout="i420"):
        """planes: CUDA uint8 [n, 1.5*H*W] (I420 or NV12) -> soft sums int64 [n, L] on device."""
        return self.engine.svd_detect_soft_yuv420(planes, height, width, payload_len, scales=self._scales, blk=self.blk, layout=layout)
