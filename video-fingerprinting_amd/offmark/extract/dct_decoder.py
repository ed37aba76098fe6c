"""DctDecoder on the MI355X.  Mirrors offmark.extract.dct_decoder.DctDecoder
(reference src/offmark/extract/dct_decoder.py:4-89): DctDecoder(key=None, alpha=20),
decode(yuv) -> float64 array (1, H*W//64) of 0./1., luminance_mask, texture_mask.  No CPU fallback."""
import numpy as np

from ..engine import DctEngine


class DctDecoder:
    def __init__(self, key=None, alpha=20):
        self.key = key
        self.alpha = alpha
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
        _counts, bits = self.engine.decode_yuv(dev, L=1, alpha=self.alpha, want_bits=True)
        return bits.cpu().numpy().astype(np.float64).reshape(1, -1)

    def _planes(self, lum):
        t = self.engine.torch
        lum = np.ascontiguousarray(lum, dtype=np.float32)
        yuv = np.zeros(lum.shape + (3,), np.float32)
        yuv[:, :, 0] = lum
        return self.engine.debug_planes(t.from_numpy(yuv).to(self.engine.device), alpha=self.alpha)

    def luminance_mask(self, lum):
        return self._planes(lum)["lum"]

    def texture_mask(self, lum):
        return self._planes(lum)["tex"]

    # -- batch fast path ---------------------------------------------------------------------------
    def bits_per_frame(self, height, width):
        """Length of decode()'s bit vector for a frame of this size (dct_decoder.py:16): what the degenerator's means divide by."""
        return height * width // 64

    def decode_frames_u8(self, frames, payload_len, want_bits=False):
        """frames: CUDA uint8 [n, H, W, 3] -> (counts int32 [n, L] on device, bits or None)."""
        return self.engine.detect(frames, payload_len, alpha=self.alpha, want_bits=want_bits)

    def decode_planes_yuv420(self, planes, height, width, payload_len, want_bits=False, layout="i420"):
        """planes: CUDA uint8 [n, 1.5*H*W] (I420 or NV12) -> (counts int32 [n, L] on device, bits or None)."""
        return self.engine.detect_yuv420(planes, height, width, payload_len, alpha=self.alpha, want_bits=want_bits, layout=layout)

    # -- soft read-out (build extension, not reference semantics: engine.detect_soft) -------------------------------------
    def decode_soft_frames_u8(self, frames, payload_len):
        """frames: CUDA uint8 [n, H, W, 3] -> soft sums int64 [n, L] on device (> 0 reads as 1)."""
        return self.engine.detect_soft(frames, payload_len, alpha=self.alpha)

    # -- block-grid resync of cropped frames (build extension, not reference semantics; offmark.resync) --------------------------
    def sync_scores_u8(self, frames):
        """frames: CUDA uint8 [n, H, W, 3], any H, W >= 8 -> int64 [n, 64] on device: per grid phase 8 * py + px the sum of
        |block metric| over the phase's full 8x8 windows, each phase under its own crop's frame mean (engine.sync_scores)."""
        return self.engine.sync_scores(frames, alpha=self.alpha)

    def decode_soft_window_u8(self, frames, L, phase, canvas_cols, base=0):
        """The soft sums int64 [n, L] of the blocks at grid ``phase``, with the positions of a frame ``canvas_cols`` blocks wide
        (engine.detect_soft_window)."""
        return self.engine.detect_soft_window(frames, L, phase, canvas_cols, base=base, alpha=self.alpha)

    # -- rescaled leaks (build extension: offmark.resync.read_rescaled_leak at a KNOWN geometry; this codec has no search) ------
    def decode_soft_warp_u8(self, frames, canvas_hw, geom, L):
        """The soft sums int64 [n, L] of the leak warped by ``geom`` onto the canvas, with the uncropped frame's positions.  The
        chain: engine.warp of the rectangle of counting units, then decode_soft_window_u8 at phase (0, 0) -- masks and frame mean
        come from the warped rectangle, as the decoder treats any received frame.  Zeros when no unit counts."""
        eng = self.engine
        H, W = int(canvas_hw[0]), int(canvas_hw[1])
        i0, i1, j0, j1 = eng.warp_units(frames.shape[1:3], (H, W), geom)
        if i1 == i0:
            return eng.torch.zeros((frames.shape[0], int(L)), dtype=eng.torch.int64, device=frames.device)
        rect = eng.warp(frames, geom, (8 * (i1 - i0), 8 * (j1 - j0)), origin=(8 * i0, 8 * j0))
        return eng.detect_soft_window(rect, L, (0, 0), W // 8, base=i0 * (W // 8) + j0, alpha=self.alpha)

    def sync_scores_planes_yuv420(self, planes, height, width, layout="i420"):
        """planes: CUDA uint8 [n, 1.5*H*W] (I420 or NV12), even H, W >= 8 -> int64 [n, 64] on device: sync_scores_u8's sums at the
        phases with even py and px, 0 elsewhere -- an odd crop offset does not exist on 4:2:0 planes (engine.sync_scores_yuv420)."""
        return self.engine.sync_scores_yuv420(planes, height, width, alpha=self.alpha, layout=layout)

    def decode_soft_window_planes_yuv420(self, planes, height, width, L, phase, canvas_cols, base=0, layout="i420"):
        """The soft sums int64 [n, L] of the blocks at the even grid ``phase``, with the positions of a frame ``canvas_cols`` blocks
        wide (engine.detect_soft_window_yuv420)."""
        return self.engine.detect_soft_window_yuv420(planes, height, width, L, phase, canvas_cols, base=base, alpha=self.alpha, layout=layout)

    def decode_soft_planes_yuv420(self, planes, height, width, payload_len, layout="i420"):
        """planes: CUDA uint8 [n, 1.5*H*W] (I420 or NV12) -> soft sums int64 [n, L] on device."""
        return self.engine.detect_soft_yuv420(planes, height, width, payload_len, alpha=self.alpha, layout=layout)
