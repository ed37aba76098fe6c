"""Batch engine over the C ABI: device tensors in, device tensors out.

This is the layer the plugin classes (DctEncoder / DctDecoder / Embedder / Extractor) and the
multi-GPU driver sit on.  It owns one scratch tensor per (H, W, frames-in-flight) and enqueues
work on torch's current stream; nothing here synchronises.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
import threading

import numpy as np

from . import _hip

# Frames per internal chunk.  Measured on MI355X (profiles/): chunks small enough to stay in the
# 256 MiB Infinity Cache between the analyze and apply passes do not pay -- short launches lose more to
# their ramps and tails than the cached second read gains (round 2, and again in round 4 with graph replay:
# 300 frames as 15 x 20 run at 214 k frames/s against 267 k in one launch) -- so chunks are as large as
# the cap allows: 8 GiB of frames by default (round 4; 2 GiB until then: config 4's 384 frames in one launch
# instead of two +2.6 %, 4K in chunks of 250-334 instead of 84 +2-5 %).  OFFMARK_CHUNK_BYTES overrides.
_CACHE_BUDGET_BYTES = int(os.environ.get("OFFMARK_CHUNK_BYTES", 8 << 30))


_MAX_CHUNK_FRAMES = 65535      # frames per launch the library accepts (gridDim.y / its own chunk clamp, csrc: kMaxChunk)


def default_chunk_frames(H: int, W: int, bytes_per_sample: int = 1) -> int:
    return max(1, min(_MAX_CHUNK_FRAMES, _CACHE_BUDGET_BYTES // (H * W * 3 * bytes_per_sample)))


def balanced_chunk(n: int, cap: int) -> int:
    """Frames per chunk when n frames are processed in chunks of at most ``cap``: the fewest chunks, all (nearly) equal --
    384 frames under a cap of 345 run as 192 + 192, not 345 + 39 (a short tail chunk pays a whole launch's ramp and tail
    for a ninth of the work: VERDICT r3, config 4 lost ~10 % to it).  Never more than the library launches at once."""
    cap = max(1, min(int(cap), _MAX_CHUNK_FRAMES))
    if n <= cap:
        return max(1, n)
    k = -(-n // cap)
    return -(-n // k)


# ---- tile order of the frame-writing DCT kernel (include/offmark_hip.h: OFMK_F_LINEAR_TILES / OFMK_F_XCD_TILES) ----------------
# No measurement anywhere.  The library applies a static rule on the bytes of frames a launch reads -- XCD-aware order from 192
# frames of 1080p per launch up, linear below -- which is what every interleaved A/B since round 3 says (large launches: the
# XCD-aware order wins by 1.5-6 % or ties, depending on where the driver put the caller's frames; 48-96 frames per launch: linear
# wins by 1-4 %; profiles/r4_mark_fused_pass.txt, profiles/r6_mark_ladder.txt).  An engine can force an order (tile_order="xcd" /
# "linear", OFFMARK_TILE_ORDER, or the caller's own ofmk_opts flags).  Rounds 4-5 also carried an opt-in per-bucket calibration;
# it steered an effect the driver's box measured at 0.15 % and is gone.  Results never depend on the order.
_TILE_ORDER_LOCK = threading.RLock()
_XCC_DEAL = {}                # device index -> probe_xcc_deal() result


def static_tile_order(launch_bytes: int) -> str:
    """The library's rule (csrc/offmark_kernels.hip: tile_xcds), restated for reporting."""
    return "xcd" if launch_bytes >= _hip.XCD_TILES_MIN_BYTES else "linear"


def probe_xcc_deal(device=None, workgroups: int = 4096) -> dict:
    """Ask the hardware which XCD each workgroup of a linear grid runs on (HW_REG_XCC_ID, ofmk_probe_xcc).
    Returns xcds (distinct ids seen), round_robin (True when workgroups L and L + xcds always share an XCD -- all the
    XCD-aware tile order assumes), ids_by_residue (the id of residue class L % xcds, in order: WHICH XCD gets workgroup 0
    is not fixed) and the fraction of workgroups that fit the round-robin pattern."""
    torch = _hip.require_gpu()
    lib = _hip.load()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    with _TILE_ORDER_LOCK:
        if key in _XCC_DEAL:
            return _XCC_DEAL[key]
        with torch.cuda.device(dev):
            ids = torch.full((workgroups,), -1, dtype=torch.int32, device=dev)
            _hip.check(lib.ofmk_probe_xcc(ids.data_ptr(), workgroups, _hip.current_stream(), None))
            got = ids.cpu().numpy()
        seen = sorted(int(v) for v in np.unique(got))
        X = len(seen)
        by_res = [int(np.bincount(got[r::X], minlength=16).argmax()) for r in range(X)]
        fit = float(np.mean(got == np.asarray(by_res)[np.arange(workgroups) % X]))
        out = dict(xcds=X, round_robin=bool(fit == 1.0 and len(set(by_res)) == X), ids_by_residue=by_res,
                   round_robin_fraction=round(fit, 4), workgroups=workgroups)
        _XCC_DEAL[key] = out
        return out


# A checked leak of a resync call: lead = the library call's leading arguments (frames, [layout,] n, H, W), suffix = its name's
_Leak = collections.namedtuple("_Leak", "lead n H W suffix")


class DctEngine:
    """Enqueue embed / detect for batches of interleaved u8 frames [n, H, W, 3] on one GPU."""

    def __init__(self, device=None, chunk_frames: int | None = None, opts=None, tile_order: str | None = None):
        """opts: an _hip.Opts applied to every batch call of this engine (flags, timing object); engines share
        no state, so two engines on two streams may be driven from two threads.
        tile_order: "auto" (default: $OFFMARK_TILE_ORDER, else "auto" = the library's static rule on the launch size) | "xcd" |
        "linear" (forced).  A pure scheduling choice: results do not depend on it."""
        self.opts = opts
        self.torch = _hip.require_gpu()
        self.lib = _hip.load()
        self.device = self.torch.device("cuda", self.torch.cuda.current_device()) if device is None \
            else self.torch.device(device)
        self.chunk_frames = chunk_frames
        order = tile_order or os.environ.get("OFFMARK_TILE_ORDER", "auto")
        if order not in ("auto", "xcd", "linear"):
            raise ValueError(f"tile_order must be 'auto', 'xcd' or 'linear', not {order!r}")
        self._order_mode = order
        self._opts_cache = None
        self._last_bytes = 0
        # range-check device-resident row maps too (costs a host synchronisation per call, so off by default; the kernels
        # clamp every entry into [0, n_wm) either way -- include/offmark_hip.h)
        self.debug_checks = os.environ.get("OFFMARK_DEBUG_CHECKS", "0") not in ("", "0")
        self._ws = {}
        self._resync_ws = {}          # slot -> (frame size, buffer): sync_workspace() / detect_soft_window(), see _side_ws

    # -- scratch ------------------------------------------------------------------------------
    def workspace(self, H: int, W: int, frames: int):
        """Scratch for `frames` frames in flight.  One buffer per frame size is kept and only ever grows: the
        library sizes its chunks to min(chunk_frames, what fits), so a larger buffer serves smaller batches."""
        nbytes = self.lib.ofmk_workspace_bytes(min(int(frames), _MAX_CHUNK_FRAMES), H, W)
        if nbytes == 0:
            raise _hip.HipError(f"bad frame size {H}x{W}")
        return self._grown_ws(H, W, nbytes)

    def copies_workspace(self, H: int, W: int, frames: int, copies: int):
        """Scratch for embed_detect_copies with `frames` frames in flight: every copy keeps its own records next to the input's
        (ofmk_copies_workspace_bytes).  The same one-buffer-per-frame-size cache as workspace(), which only grows."""
        nbytes = self.lib.ofmk_copies_workspace_bytes(min(int(frames), _MAX_CHUNK_FRAMES), int(copies), H, W)
        if nbytes == 0:
            raise _hip.HipError(f"bad frame size {H}x{W} or copies {copies}")
        return self._grown_ws(H, W, nbytes)

    def _grown_ws(self, H, W, nbytes):
        ws = self._ws.get((H, W))
        if ws is None or ws.numel() < nbytes:
            ws = self.torch.empty(nbytes, dtype=self.torch.uint8, device=self.device)
            self._ws = {(H, W): ws}       # keep one size; frame sizes rarely change within a job
        return ws

    def place_buffers(self, frames, want_out: bool = True, candidates: int = 8):
        """Set-up for a device-resident batch path: pick this engine's workspace -- and, ``want_out``, a destination for the marked
        frames -- among ``candidates`` allocations by the real kernels' launch time over ``frames`` (offmark/placement.py: the
        buffers the kernels WRITE decide which of three speed levels they run at on MI355X, 3-10 % apart; a buffer keeps its level
        while it lives).  Returns (out tensor or None, report).  Synchronises; call once, before capturing graphs; results never
        depend on it."""
        from .placement import place_buffers
        return place_buffers(self, frames, want_out=want_out, candidates=candidates)

    def _chunk(self, n, H, W, bytes_per_sample=1):
        """Frames per internal chunk: equal chunks under the cap (chunk_frames or the byte budget)."""
        return balanced_chunk(n, self.chunk_frames or default_chunk_frames(H, W, bytes_per_sample))

    # -- tile order ------------------------------------------------------------------------------
    @property
    def device_key(self):
        return self.device.index if self.device.index is not None else self.torch.cuda.current_device()

    @property
    def tile_order(self) -> str:
        """The order the last marking call ran in: this engine's (or its opts') forced choice, else the static rule for that
        call's launch size."""
        if self._order_mode in ("xcd", "linear"):
            return self._order_mode
        return self._pinned() or static_tile_order(self._last_bytes)

    @property
    def tile_order_info(self) -> dict:
        policy = "forced" if self._order_mode in ("xcd", "linear") or self._pinned() else "static rule"
        return dict(mode=self._order_mode, in_use=self.tile_order, policy=policy, launch_bytes=self._last_bytes,
                    static_rule=static_tile_order(self._last_bytes), xcd_from_bytes=_hip.XCD_TILES_MIN_BYTES)

    def _pinned(self):
        """The order the caller's own opts force, if any."""
        if self.opts is None:
            return None
        if self.opts.flags & _hip.F_LINEAR_TILES or self.opts.xcds == 1:
            return "linear"
        if self.opts.flags & _hip.F_XCD_TILES:
            return "xcd"
        return None

    def _o(self, launch_bytes=None, extra_flags=0):
        """ctypes argument for this call's ofmk_opts: the engine's opts (flags, timing) plus, for a call that runs the frame-writing
        DCT kernel (``launch_bytes`` = bytes of frames per launch), the engine's forced tile order, if it has one (else none: the
        library's static rule); ``extra_flags``: flags of this one call (OFMK_F_PARTIAL_COUNTS)."""
        base = self.opts
        flags = (base.flags if base is not None else 0) | extra_flags
        xcds = base.xcds if base is not None else 0
        if launch_bytes is not None:
            self._last_bytes = int(launch_bytes)
            if not self._pinned():
                if self._order_mode == "linear":
                    flags |= _hip.F_LINEAR_TILES
                elif self._order_mode == "xcd":
                    flags |= _hip.F_XCD_TILES
        if base is not None and flags == base.flags and xcds == base.xcds:
            return _hip.opts_ref(base)
        if flags == 0 and xcds == 0 and base is None:
            return None
        o = _hip.Opts(flags, xcds, base.timing if base is not None else None)
        self._opts_cache = o                                  # alive until the next call
        return _hip.opts_ref(o)

    def _check_frames(self, frames, dtype):
        t = self.torch
        if not (isinstance(frames, t.Tensor) and frames.is_cuda and frames.dtype == dtype
                and frames.dim() == 4 and frames.shape[3] == 3 and frames.is_contiguous()):
            raise ValueError(f"frames must be a contiguous CUDA tensor [n,H,W,3] of {dtype}")
        n, H, W, _ = frames.shape
        return n, H, W

    def _buffer(self, name, given, shape, dtype, device):
        """An output of a call: a fresh tensor, or the caller's, which must be a contiguous CUDA tensor of exactly this shape,
        dtype and device -- the kernels write through its raw pointer."""
        t = self.torch
        shape = tuple(shape)
        if given is None:
            return t.empty(shape, dtype=dtype, device=device)
        if not (isinstance(given, t.Tensor) and given.is_cuda and given.device == device and given.dtype == dtype
                and tuple(given.shape) == shape and given.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous CUDA {dtype} tensor of shape {shape} on {device}")
        return given

    def _out(self, out, like, shape=None):
        """The destination of a call: the expected shape (default: ``like``'s), ``like``'s dtype and device."""
        return self._buffer("out", out, like.shape if shape is None else shape, like.dtype, like.device)

    def _counts(self, counts, n, L, copies=None):
        """The position sums of a call: a fresh int32 [n, L] tensor, or the caller's (a pipeline that hands them to another
        stream keeps its own buffers: torch's allocator would hand a per-call tensor's block out again on the issuing stream).
        ``copies``: one such array per copy, [copies, n, L]."""
        return self._buffer("counts", counts, (n, L) if copies is None else (copies, n, L), self.torch.int32, self.device)

    def _soft(self, soft, n, L, copies=None):
        """The soft sums of a call: a fresh int64 [n, L] tensor, or the caller's (whatever it holds: the library clears it).
        ``copies``: one such array per copy, [copies, n, L]; ``soft`` may then be True (a fresh tensor)."""
        shape = (n, L) if copies is None else (copies, n, L)
        return self._buffer("soft", None if soft is True else soft, shape, self.torch.int64, self.device)

    def _on_device(self, x, dtype):
        """A small input of a call (``dtype``: the name numpy and torch share): the tensor on this device, or an array copied there."""
        t = self.torch
        if not isinstance(x, t.Tensor):
            x = t.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dtype)))
        return x.to(device=self.device, dtype=getattr(t, dtype)).contiguous()

    def _cands(self, cands, cols):
        """The candidate list of a search call -> (int64 [K, cols] on this device, K)."""
        cands = self._on_device(cands, "int64")
        if cands.dim() != 2 or cands.shape[1] != cols or cands.shape[0] < 1:
            raise ValueError(f"cands must be int64 [K, {cols}] with K >= 1")
        return cands, int(cands.shape[0])

    def _layout(self, layout):
        try:
            return self._LAYOUT[layout]
        except KeyError:
            raise ValueError(f"unknown 4:2:0 layout {layout!r}: one of {sorted(self._LAYOUT)}") from None

    def _wm(self, wm, N):
        t = self.torch
        if isinstance(wm, np.ndarray):
            wm = t.from_numpy(np.ascontiguousarray(wm.reshape(-1, N)).astype(np.uint8)).to(self.device)
        wm = wm.reshape(-1, N)
        if wm.dtype != t.uint8 or not wm.is_cuda or not wm.is_contiguous():
            wm = wm.to(device=self.device, dtype=t.uint8).contiguous()
        return wm

    def _rows(self, wm_row, n, n_wm=None):
        """Per-frame watermark-row map -> device int32 [n].  Host arrays are always range-checked here, device tensors
        when ``debug_checks`` is set (OFFMARK_DEBUG_CHECKS=1: it needs a synchronisation); the kernels clamp whatever
        arrives into [0, n_wm), so a bad map marks with the wrong row but never reads out of bounds."""
        if wm_row is None:
            return None
        t = self.torch
        if isinstance(wm_row, (list, tuple)):
            wm_row = np.asarray(wm_row)
        if isinstance(wm_row, np.ndarray):
            if n_wm is not None and wm_row.size and (wm_row.min() < 0 or wm_row.max() >= n_wm):
                raise ValueError(f"wm_row entries must be in [0, {n_wm}); got [{wm_row.min()}, {wm_row.max()}]")
            wm_row = t.from_numpy(wm_row.astype(np.int32))
        elif (n_wm is not None and (not wm_row.is_cuda or self.debug_checks) and wm_row.numel()
              and (int(wm_row.min()) < 0 or int(wm_row.max()) >= n_wm)):
            raise ValueError(f"wm_row entries must be in [0, {n_wm}); got [{int(wm_row.min())}, {int(wm_row.max())}]")
        wm_row = wm_row.to(device=self.device, dtype=t.int32).contiguous()
        if wm_row.numel() != n:
            raise ValueError("wm_row needs one entry per frame")
        return wm_row

    # -- u8 RGB batch path (the hot path) --------------------------------------------------------
    def embed(self, frames, wm, alpha=20, wm_row=None, out=None):
        """Mark every frame.  wm: (n_wm, N) 0/1 array or tensor; wm_row: per-frame row of wm."""
        t = self.torch
        n, H, W = self._check_frames(frames, t.uint8)
        N = H * W // 64
        wm = self._wm(wm, N)
        rows = self._rows(wm_row, n, wm.shape[0])
        out = self._out(out, frames)
        cf = self._chunk(n, H, W)
        ws = self.workspace(H, W, cf)
        _hip.check(self.lib.ofmk_embed_rgb8(frames.data_ptr(), out.data_ptr(), n, H, W, wm.data_ptr(), wm.shape[0],
                                            _hip.ptr(rows), float(alpha), cf, ws.data_ptr(), ws.numel(), _hip.current_stream(),
                                            self._o(min(cf, n) * H * W * 3)))
        return out

    def detect(self, frames, L, alpha=20, want_bits=False, counts=None):
        """Returns (counts int32 [n, L], bits u8 [n, N] or None)."""
        t = self.torch
        n, H, W = self._check_frames(frames, t.uint8)
        N = H * W // 64
        counts = self._counts(counts, n, L)
        bits = t.empty((n, N), dtype=t.uint8, device=self.device) if want_bits else None
        cf = self._chunk(n, H, W)
        ws = self.workspace(H, W, cf)
        _hip.check(self.lib.ofmk_detect_rgb8(frames.data_ptr(), n, H, W, int(L), float(alpha), counts.data_ptr(),
                                             _hip.ptr(bits), cf, ws.data_ptr(), ws.numel(), _hip.current_stream(),
                                             self._o()))
        return counts, bits

    def detect_soft(self, frames, L, alpha=20, soft=None):
        """Build extension (not reference semantics): per-position soft sums, int64 [n, L]; > 0 reads as 1."""
        t = self.torch
        n, H, W = self._check_frames(frames, t.uint8)
        soft = self._soft(soft, n, L)
        cf = self._chunk(n, H, W)
        ws = self.workspace(H, W, cf)
        _hip.check(self.lib.ofmk_detect_soft_rgb8(frames.data_ptr(), n, H, W, int(L), float(alpha), soft.data_ptr(), cf,
                                                  ws.data_ptr(), ws.numel(), _hip.current_stream(), self._o()))
        return soft

    # -- block-grid resync of cropped frames (build extension, not reference semantics; offmark.resync) ------------------------
    def _side_ws(self, slot, key, nbytes):
        """A scratch buffer of the resync calls, cached per ``slot`` next to -- never in place of -- workspace()'s buffer: one
        frame size per slot, only ever growing."""
        held = self._resync_ws.get(slot)
        if held is None or held[0] != key or held[1].numel() < nbytes:
            held = (key, self.torch.empty(nbytes, dtype=self.torch.uint8, device=self.device))
            self._resync_ws[slot] = held
        return held[1]

    def _sync_ws(self, slot, sizing, H, W, frames):
        nbytes = sizing(min(int(frames), _MAX_CHUNK_FRAMES), H, W)
        if nbytes == 0:
            raise _hip.HipError(f"bad frame size {H}x{W}")
        return self._side_ws(slot, (H, W), nbytes)

    def _window_ws(self, slot, cf, H, W, py, px):
        """Scratch of a DCT window read-out: workspace() bytes for the window's blocks at phase (py, px)."""
        if 0 <= py <= 7 and 0 <= px <= 7 and H - py >= 8 and W - px >= 8:
            h8, w8 = (H - py) // 8 * 8, (W - px) // 8 * 8
            return self._side_ws(slot, (h8, w8), self.lib.ofmk_workspace_bytes(min(cf, _MAX_CHUNK_FRAMES), h8, w8))
        return self._side_ws(slot, (8, 8), self.lib.ofmk_workspace_bytes(1, 8, 8))       # the library refuses the phase

    # The resync calls come as an RGB and a 4:2:0 method with one private body: the leak descriptor carries what differs, the
    # library call's leading arguments and its name's suffix.
    def _rgb_leak(self, frames):
        n, H, W = self._check_frames(frames, self.torch.uint8)
        return _Leak((frames.data_ptr(), n, H, W), n, H, W, "rgb8")

    def _planar_leak(self, planes, H, W, layout):
        n = self._check_planar_even(planes, H, W)
        return _Leak((planes.data_ptr(), self._layout(layout), n, H, W), n, H, W, "yuv420")

    def _resync_call(self, name, leak, *args):
        _hip.check(getattr(self.lib, f"ofmk_{name}_{leak.suffix}")(*leak.lead, *args, _hip.current_stream(), self._o()))

    def _sync_scores(self, leak, share, workspace, alpha, scores):
        """share: the part of the frame budget a chunk takes, so that its records stay at the frames' size."""
        scores = self._soft(scores, leak.n, 64)
        cf = balanced_chunk(leak.n, max(1, (self.chunk_frames or default_chunk_frames(leak.H, leak.W)) // share))
        ws = workspace(leak.H, leak.W, cf)
        self._resync_call("sync_scores", leak, float(alpha), scores.data_ptr(), cf, ws.data_ptr(), ws.numel())
        return scores

    def _detect_soft_window(self, leak, slot, L, phase, canvas_cols, base, alpha, soft):
        soft = self._soft(soft, leak.n, L)
        py, px = (int(v) for v in phase)
        cf = self._chunk(leak.n, leak.H, leak.W)
        ws = self._window_ws(slot, cf, leak.H, leak.W, py, px)
        self._resync_call("detect_soft_window", leak, py, px, int(canvas_cols), int(base), int(L), float(alpha), soft.data_ptr(), cf,
                          ws.data_ptr(), ws.numel())
        return soft

    def _svd_sync_scores(self, leak, scale, scales, blk, scores):
        scores = self._soft(scores, leak.n, 64)
        self._resync_call("svd_sync_scores", leak, _hip.scales3(scale, scales), int(blk), scores.data_ptr())
        return scores

    def _svd_detect_soft_window(self, leak, L, phase, canvas_cols, base, scale, scales, blk, soft):
        soft = self._soft(soft, leak.n, L)
        py, px = phase
        self._resync_call("svd_detect_soft_window", leak, int(py), int(px), int(canvas_cols), int(base), int(L), _hip.scales3(scale, scales),
                          int(blk), soft.data_ptr())
        return soft

    def sync_workspace(self, H: int, W: int, frames: int):
        """Scratch of sync_scores for `frames` frames in flight (ofmk_sync_workspace_bytes: one record per pixel origin).  A cache
        of its own: the ordinary workspace() buffer is neither replaced nor freed."""
        return self._sync_ws("sync", self.lib.ofmk_sync_workspace_bytes, H, W, frames)

    def sync_scores(self, frames, alpha=20, scores=None):
        """The dense phase search: int64 [n, 64], entry 8 * py + px = the sum of |block metric| over the full 8x8 windows of the
        frame at grid phase (py, px), i.e. ``detect_soft(crop, blocks, alpha).abs().sum(1)`` of the contiguous crop that holds the
        phase's blocks -- masks and frame mean taken from that crop -- integer for integer.  H and W are any values >= 8.
        offmark.resync.best_phase reads it."""
        # 12 bytes per pixel origin against 3 per pixel: a quarter of the frame budget keeps the records at the frames' size
        return self._sync_scores(self._rgb_leak(frames), 4, self.sync_workspace, alpha, scores)

    def detect_soft_window(self, frames, L, phase, canvas_cols, base=0, alpha=20, soft=None):
        """detect_soft of the blocks at grid ``phase`` = (py, px): block (i, j) is the 8x8 block at pixel (py + 8i, px + 8j) and
        adds into position (base + i * canvas_cols + j) % L, the position it has in a frame ``canvas_cols`` blocks wide.  Masks
        and frame mean come from the window.  int64 [n, L]."""
        return self._detect_soft_window(self._rgb_leak(frames), "window", L, phase, canvas_cols, base, alpha, soft)

    def embed_detect(self, frames, wm, L, alpha=20, wm_row=None, out=None, want_bits=False, counts=None):
        """Mark, then read back the marked frames chunk by chunk (mark + verify)."""
        t = self.torch
        n, H, W = self._check_frames(frames, t.uint8)
        N = H * W // 64
        wm = self._wm(wm, N)
        rows = self._rows(wm_row, n, wm.shape[0])
        out = self._out(out, frames)
        counts = self._counts(counts, n, L)
        bits = t.empty((n, N), dtype=t.uint8, device=self.device) if want_bits else None
        cf = self._chunk(n, H, W)
        ws = self.workspace(H, W, cf)
        _hip.check(self.lib.ofmk_embed_detect_rgb8(frames.data_ptr(), out.data_ptr(), n, H, W, wm.data_ptr(),
                                                   wm.shape[0], _hip.ptr(rows), float(alpha), int(L),
                                                   counts.data_ptr(), _hip.ptr(bits), cf, ws.data_ptr(), ws.numel(),
                                                   _hip.current_stream(), self._o(min(cf, n) * H * W * 3)))
        return out, counts, bits

    def payloads(self, counts, n_bits: int, perm, out=None, counts_out=None):
        """Device epilogue of DeShuffler.degenerate for a batch: counts int32 [n, L] -> uint8 [n, L].  ``counts`` may also be
        the PARTIAL form int32 [n, tiles, L] a DwtDctSvd read-out left with ``partial=True`` (every frame-kernel workgroup's own
        sums, stored not added): the tiles are added up inside the same kernel, and ``counts_out`` (int32 [n, L], optional)
        receives the sums."""
        t = self.torch
        if not isinstance(perm, t.Tensor):
            perm = t.as_tensor(np.asarray(perm), dtype=t.int32).to(self.device)
        if counts.dim() == 3:
            n, tiles, L = counts.shape
            if out is None:
                out = t.empty((n, L), dtype=t.uint8, device=self.device)
            _hip.check(self.lib.ofmk_payloads_from_partial_counts(counts.data_ptr(), tiles, n, L, int(n_bits), perm.data_ptr(), out.data_ptr(),
                                                                  _hip.ptr(counts_out), _hip.current_stream(), self._o()))
            return out
        n, L = counts.shape
        if out is None:
            out = t.empty((n, L), dtype=t.uint8, device=self.device)
        _hip.check(self.lib.ofmk_payloads_from_counts(counts.data_ptr(), n, L, int(n_bits), perm.data_ptr(),
                                                      out.data_ptr(), _hip.current_stream(), self._o()))
        return out

    def counts_from_partial(self, partials, out=None):
        """The frames' [n, L] counts from partial counts [n, tiles, L] (one small kernel; integer sums)."""
        t = self.torch
        n, tiles, L = partials.shape
        out = self._counts(out, n, L)
        _hip.check(self.lib.ofmk_payloads_from_partial_counts(partials.data_ptr(), tiles, n, L, 0, None, None, out.data_ptr(),
                                                              _hip.current_stream(), self._o()))
        return out

    # -- planar 8-bit YUV 4:2:0 in and out (what a decoder hands over / an encoder takes) -----------
    _LAYOUT = {"i420": _hip.YUV_I420, "nv12": _hip.YUV_NV12}

    def _check_planar(self, planes, H, W):
        t = self.torch
        if H % 8 or W % 8:
            raise ValueError("planar 4:2:0 frames need H and W to be multiples of 8")
        if not (isinstance(planes, t.Tensor) and planes.is_cuda and planes.dtype == t.uint8 and planes.dim() == 2
                and planes.shape[1] == H * W * 3 // 2 and planes.is_contiguous()):
            raise ValueError("planes must be a contiguous CUDA uint8 tensor [n, H*W*3/2] (I420: Y|U|V, NV12: Y|UV per frame)")
        return planes.shape[0]

    def embed_yuv420(self, planes, H, W, wm, alpha=20, wm_row=None, out=None, layout="i420"):
        """Mark frames given as 4:2:0 planes [n, 1.5*H*W]; returns marked planes of the same layout.  Equal, bit for
        bit, to yuv420_to_rgb -> embed -> rgb_to_yuv420 with the build-defined conversion."""
        t = self.torch
        n = self._check_planar(planes, H, W)
        wm = self._wm(wm, H * W // 64)
        rows = self._rows(wm_row, n, wm.shape[0])
        out = self._out(out, planes)
        cf = self._chunk(n, H, W)
        ws = self.workspace(H, W, cf)
        _hip.check(self.lib.ofmk_embed_yuv420(planes.data_ptr(), out.data_ptr(), self._layout(layout), n, H, W, wm.data_ptr(),
                                              wm.shape[0], _hip.ptr(rows), float(alpha), cf, ws.data_ptr(), ws.numel(),
                                              _hip.current_stream(), self._o()))
        return out

    def detect_yuv420(self, planes, H, W, L, alpha=20, want_bits=False, layout="i420"):
        t = self.torch
        n = self._check_planar(planes, H, W)
        counts = t.empty((n, L), dtype=t.int32, device=self.device)
        bits = t.empty((n, H * W // 64), dtype=t.uint8, device=self.device) if want_bits else None
        cf = self._chunk(n, H, W)
        ws = self.workspace(H, W, cf)
        _hip.check(self.lib.ofmk_detect_yuv420(planes.data_ptr(), self._layout(layout), n, H, W, int(L), float(alpha),
                                               counts.data_ptr(), _hip.ptr(bits), cf, ws.data_ptr(), ws.numel(),
                                               _hip.current_stream(), self._o()))
        return counts, bits

    def detect_soft_yuv420(self, planes, H, W, L, alpha=20, layout="i420", soft=None):
        """Build extension (not reference semantics): detect_soft on 4:2:0 planes, int64 [n, L]; equal, integer for integer,
        to detect_soft(yuv420_to_rgb(planes))."""
        n = self._check_planar(planes, H, W)
        soft = self._soft(soft, n, L)
        cf = self._chunk(n, H, W)
        ws = self.workspace(H, W, cf)
        _hip.check(self.lib.ofmk_detect_soft_yuv420(planes.data_ptr(), self._layout(layout), n, H, W, int(L), float(alpha),
                                                    soft.data_ptr(), cf, ws.data_ptr(), ws.numel(), _hip.current_stream(), self._o()))
        return soft

    def embed_detect_yuv420(self, planes, H, W, wm, L, alpha=20, wm_row=None, out=None, want_bits=False, layout="i420", counts=None):
        """Mark and verify on planes; counts/bits are what a reader of the WRITTEN planes gets."""
        t = self.torch
        n = self._check_planar(planes, H, W)
        wm = self._wm(wm, H * W // 64)
        rows = self._rows(wm_row, n, wm.shape[0])
        out = self._out(out, planes)
        counts = self._counts(counts, n, L)
        bits = t.empty((n, H * W // 64), dtype=t.uint8, device=self.device) if want_bits else None
        cf = self._chunk(n, H, W)
        ws = self.workspace(H, W, cf)
        _hip.check(self.lib.ofmk_embed_detect_yuv420(planes.data_ptr(), out.data_ptr(), self._layout(layout), n, H, W,
                                                     wm.data_ptr(), wm.shape[0], _hip.ptr(rows), float(alpha), int(L),
                                                     counts.data_ptr(), _hip.ptr(bits), cf, ws.data_ptr(), ws.numel(),
                                                     _hip.current_stream(), self._o()))
        return out, counts, bits

    def yuv420_to_rgb(self, planes, H, W, layout="i420", out=None):
        t = self.torch
        n = self._check_planar(planes, H, W)
        rgb = self._out(out, planes, (n, H, W, 3))
        _hip.check(self.lib.ofmk_yuv420_to_rgb8(planes.data_ptr(), rgb.data_ptr(), self._layout(layout), n, H, W,
                                                _hip.current_stream(), self._o()))
        return rgb

    def rgb_to_yuv420(self, frames, layout="i420", out=None):
        t = self.torch
        n, H, W = self._check_frames(frames, t.uint8)
        if H % 8 or W % 8:
            raise ValueError("planar 4:2:0 frames need H and W to be multiples of 8")
        planes = self._out(out, frames, (n, H * W * 3 // 2))
        _hip.check(self.lib.ofmk_rgb8_to_yuv420(frames.data_ptr(), planes.data_ptr(), self._layout(layout), n, H, W,
                                                _hip.current_stream(), self._o()))
        return planes

    # -- float32 YUV path (the literal encode(yuv)/decode(yuv) plugin boundary) ------------------
    def encode_yuv(self, yuv, wm, alpha=20, wm_row=None):
        t = self.torch
        n, H, W = self._check_frames(yuv, t.float32)
        wm = self._wm(wm, H * W // 64)
        rows = self._rows(wm_row, n, wm.shape[0])
        cf = self._chunk(n, H, W, bytes_per_sample=4)
        ws = self.workspace(H, W, cf)
        _hip.check(self.lib.ofmk_encode_yuv32f(yuv.data_ptr(), n, H, W, wm.data_ptr(), wm.shape[0], _hip.ptr(rows),
                                               float(alpha), cf, ws.data_ptr(), ws.numel(), _hip.current_stream(), self._o()))
        return yuv

    def decode_yuv(self, yuv, L=1, alpha=20, want_bits=True):
        t = self.torch
        n, H, W = self._check_frames(yuv, t.float32)
        N = H * W // 64
        counts = t.empty((n, L), dtype=t.int32, device=self.device)
        bits = t.empty((n, N), dtype=t.uint8, device=self.device) if want_bits else None
        cf = self._chunk(n, H, W, bytes_per_sample=4)
        ws = self.workspace(H, W, cf)
        _hip.check(self.lib.ofmk_decode_yuv32f(yuv.data_ptr(), n, H, W, int(L), float(alpha), counts.data_ptr(),
                                               _hip.ptr(bits), cf, ws.data_ptr(), ws.numel(), _hip.current_stream(), self._o()))
        return counts, bits

    # -- DwtDctSvd codec (one pass, no workspace) ---------------------------------------------------
    @staticmethod
    def svd_bits_per_frame(H, W, blk=4):
        """Length of the decoder's bit array (dwt_dct_svd_decoder.py:14): row*col//4//(blk*blk)."""
        return H * W // 4 // (blk * blk)

    def svd_embed(self, frames, wm, scale=15, wm_row=None, out=None, scales=None, blk=4):
        t = self.torch
        n, H, W = self._check_frames(frames, t.uint8)
        wm = self._wm(wm, H * W // 64)
        rows = self._rows(wm_row, n, wm.shape[0])
        out = self._out(out, frames)
        _hip.check(self.lib.ofmk_svd_embed_rgb8(frames.data_ptr(), out.data_ptr(), n, H, W, wm.data_ptr(), wm.shape[0],
                                                _hip.ptr(rows), _hip.scales3(scale, scales), int(blk), _hip.current_stream(),
                                                self._o()))
        return out

    def _svd_counts(self, counts, n, H, W, L, blk, partial, copies=None):
        """The read-out's counts buffer: [n, L] (cleared by the library, added into with atomics) or, ``partial``, the
        per-workgroup form [n, tiles, L] the frame kernel stores in full -- no fill dispatch in front of it
        (include/offmark_hip.h: OFMK_F_PARTIAL_COUNTS; L <= 2048); hand it to payloads() / counts_from_partial().
        ``copies``: one such buffer per copy, [copies, n, ...].  Returns (counts, the flag for the call's opts)."""
        shape, flag = (n, int(L)), 0
        if partial:
            tiles = int(self.lib.ofmk_svd_count_tiles(H, W, int(blk)))
            if tiles < 0:
                raise _hip.HipError(f"bad frame size or blk ({H}x{W}, blk={blk})")
            shape, flag = (n, tiles, int(L)), _hip.F_PARTIAL_COUNTS
        if copies is not None:
            shape = (copies,) + shape
        return self._buffer("counts", counts, shape, self.torch.int32, self.device), flag

    def svd_detect(self, frames, L, scale=15, want_bits=False, scales=None, blk=4, counts=None, partial=False):
        t = self.torch
        n, H, W = self._check_frames(frames, t.uint8)
        counts, flag = self._svd_counts(counts, n, H, W, L, blk, partial)
        bits = t.empty((n, self.svd_bits_per_frame(H, W, blk)), dtype=t.uint8, device=self.device) if want_bits else None
        _hip.check(self.lib.ofmk_svd_detect_rgb8(frames.data_ptr(), n, H, W, int(L), _hip.scales3(scale, scales), int(blk), counts.data_ptr(),
                                                 _hip.ptr(bits), _hip.current_stream(), self._o(extra_flags=flag)))
        return counts, bits

    def svd_detect_soft(self, frames, L, scale=15, scales=None, blk=4, soft=None):
        """Build extension (not reference semantics): the DwtDctSvd read-out's soft sums, int64 [n, L].  Per unit (8x8 pixel
        block for blk 4, 16x16 tile for blk 8) round(-sin(2 pi s0 / scale) * 2^14), summed over the units c with c % L == i:
        > 0 reads as 1, the sign agrees with svd_detect's bit, sums over frames may be added (dist.vote.soft_vote)."""
        t = self.torch
        n, H, W = self._check_frames(frames, t.uint8)
        soft = self._soft(soft, n, L)
        _hip.check(self.lib.ofmk_svd_detect_soft_rgb8(frames.data_ptr(), n, H, W, int(L), _hip.scales3(scale, scales), int(blk),
                                                      soft.data_ptr(), _hip.current_stream(), self._o()))
        return soft

    # -- block-grid resync of cropped frames (build extension, not reference semantics; blk 4, channel 1; offmark.resync) --------
    def svd_sync_scores(self, frames, scale=15, scales=None, blk=4, scores=None):
        """The dense phase search: int64 [n, 64], entry 8 * py + px = the sum of |unit metric| (svd_detect_soft's, blk 4) over the
        full 8x8 windows of the frame at grid phase (py, px).  H and W are any values >= 8.  offmark.resync.best_phase reads it."""
        return self._svd_sync_scores(self._rgb_leak(frames), scale, scales, blk, scores)

    def svd_detect_soft_window(self, frames, L, phase, canvas_cols, base=0, scale=15, scales=None, blk=4, soft=None):
        """svd_detect_soft of the units at grid ``phase`` = (py, px): unit (i, j) is the 8x8 block at pixel (py + 8i, px + 8j) and
        adds into position (base + i * canvas_cols + j) % L, the position it has in a frame ``canvas_cols`` units wide.  int64 [n, L]."""
        return self._svd_detect_soft_window(self._rgb_leak(frames), L, phase, canvas_cols, base, scale, scales, blk, soft)

    # -- rescaled leaks: fixed-point warp onto the marked frame's canvas (build extension; blk 4, channel 1; offmark.resync) -----
    @staticmethod
    def _warp_geom(geom):
        g = [int(v) for v in np.asarray(geom).reshape(-1)]
        if len(g) != 4:
            raise ValueError("a warp geometry is (ay, by, ax, bx) in Q16")
        return _hip.Warp(*g)

    def warp(self, frames, geom, out_hw, origin=(0, 0), out=None):
        """The leak ``frames`` (uint8 [n, h, w, 3]) resampled by ``geom`` = (ay, by, ax, bx) (Q16; offmark.resync.warp_of_crop) onto
        the canvas rectangle of ``out_hw`` pixels whose top-left canvas pixel is ``origin``: uint8 [n, Hout, Wout, 3], 0 outside the
        leak.  Integer bilinear (include/offmark_hip.h: ofmk_warp)."""
        t = self.torch
        n, h, w = self._check_frames(frames, t.uint8)
        Hout, Wout = (int(v) for v in out_hw)
        out = self._out(out, frames, (n, Hout, Wout, 3))
        g = self._warp_geom(geom)
        _hip.check(self.lib.ofmk_warp_rgb8(frames.data_ptr(), n, h, w, out.data_ptr(), Hout, Wout, int(origin[0]), int(origin[1]), C.byref(g),
                                           _hip.current_stream(), self._o()))
        return out

    def warp_units(self, leak_hw, canvas_hw, geom):
        """(i0, i1, j0, j1): the rectangle of canvas units whose 64 pixels all fall inside the leak under ``geom``; all 0 when none
        does.  Host only."""
        r = (C.c_int * 4)()
        g = self._warp_geom(geom)
        _hip.check(self.lib.ofmk_warp_units(int(leak_hw[0]), int(leak_hw[1]), int(canvas_hw[0]), int(canvas_hw[1]), C.byref(g), r))
        return tuple(r)

    def svd_warp_scores(self, frames, canvas_hw, cands, scale=15, scales=None, blk=4, scores=None):
        """The geometry search over a candidate list: int64 [n, K], entry k = the sum of |unit metric| (svd_detect_soft's, blk 4)
        over the counting units of the frame warped by cands[k].  ``cands``: int64 [K, 4] rows (ay, by, ax, bx), a tensor on this
        device or an array (copied there).  No warped frame is written.  offmark.resync.best_geometry reads the result."""
        t = self.torch
        n, h, w = self._check_frames(frames, t.uint8)
        cands, K = self._cands(cands, 4)
        scores = self._soft(scores, n, K)
        _hip.check(self.lib.ofmk_svd_warp_scores_rgb8(frames.data_ptr(), n, h, w, int(canvas_hw[0]), int(canvas_hw[1]), cands.data_ptr(), K,
                                                      _hip.scales3(scale, scales), int(blk), scores.data_ptr(), _hip.current_stream(),
                                                      self._o()))
        return scores

    def svd_detect_soft_warp(self, frames, canvas_hw, geom, L, scale=15, scales=None, blk=4, soft=None):
        """svd_detect_soft of the leak warped by ``geom`` onto a canvas of ``canvas_hw`` pixels, counting units only, unit (i, j) at
        the position it has in the uncropped frame, (i * (W // 8) + j) % L.  int64 [n, L]; equals warp + svd_detect_soft_window."""
        t = self.torch
        n, h, w = self._check_frames(frames, t.uint8)
        soft = self._soft(soft, n, L)
        g = self._warp_geom(geom)
        _hip.check(self.lib.ofmk_svd_detect_soft_warp_rgb8(frames.data_ptr(), n, h, w, int(canvas_hw[0]), int(canvas_hw[1]), C.byref(g), int(L),
                                                           _hip.scales3(scale, scales), int(blk), soft.data_ptr(), _hip.current_stream(),
                                                           self._o()))
        return soft

    # -- rotated leaks: the same warp under a 2x3 affine map (build extension; blk 4, channel 1; offmark.resync) ------------------
    @staticmethod
    def _affine_geom(geom):
        g = [int(v) for v in np.asarray(geom).reshape(-1)]
        if len(g) != 6:
            raise ValueError("an affine geometry is (ayy, ayx, by, axy, axx, bx) in Q16")
        return _hip.Affine(*g)

    def warp_affine(self, frames, geom, out_hw, origin=(0, 0), out=None):
        """``warp`` under ``geom`` = (ayy, ayx, by, axy, axx, bx) (Q16; offmark.resync.affine_of_rotation): canvas pixel (y, x) reads
        the leak at (ayy * y + ayx * x + by, axy * y + axx * x + bx).  uint8 [n, Hout, Wout, 3], 0 outside the leak
        (include/offmark_hip.h: ofmk_affine)."""
        t = self.torch
        n, h, w = self._check_frames(frames, t.uint8)
        Hout, Wout = (int(v) for v in out_hw)
        out = self._out(out, frames, (n, Hout, Wout, 3))
        g = self._affine_geom(geom)
        _hip.check(self.lib.ofmk_warp_affine_rgb8(frames.data_ptr(), n, h, w, out.data_ptr(), Hout, Wout, int(origin[0]), int(origin[1]),
                                                  C.byref(g), _hip.current_stream(), self._o()))
        return out

    def affine_units(self, leak_hw, canvas_hw, geom):
        """(i0, i1, j0, j1, count): the bounding rectangle of the canvas units whose 64 pixels all fall inside the leak under
        ``geom``, and how many there are (they are convex, not a rectangle); all 0 when none does.  Host only."""
        r = (C.c_int * 5)()
        g = self._affine_geom(geom)
        _hip.check(self.lib.ofmk_affine_units(int(leak_hw[0]), int(leak_hw[1]), int(canvas_hw[0]), int(canvas_hw[1]), C.byref(g), r))
        return tuple(r)

    def svd_affine_scores(self, frames, canvas_hw, cands, scale=15, scales=None, blk=4, scores=None):
        """svd_warp_scores over affine candidates: ``cands`` int64 [K, 6] rows (ayy, ayx, by, axy, axx, bx), a tensor on this
        device or an array (copied there).  int64 [n, K]; a candidate out of range or without a counting unit scores 0."""
        t = self.torch
        n, h, w = self._check_frames(frames, t.uint8)
        cands, K = self._cands(cands, 6)
        scores = self._soft(scores, n, K)
        _hip.check(self.lib.ofmk_svd_affine_scores_rgb8(frames.data_ptr(), n, h, w, int(canvas_hw[0]), int(canvas_hw[1]), cands.data_ptr(), K,
                                                        _hip.scales3(scale, scales), int(blk), scores.data_ptr(), _hip.current_stream(),
                                                        self._o()))
        return scores

    def svd_affine_phase_scores(self, frames, canvas_hw, cands, scale=15, scales=None, blk=4, scores=None, units=None):
        """The dense shift search: svd_affine_scores of every candidate under all 64 whole-pixel shifts (py, px) in 0..7 of the
        canvas (offmark.resync.shift_affine), for about the price of one.  -> (scores int64 [n, K, 64], units int64 [K, 64]), at
        index 8 * py + px: the sum of |unit metric| and the number of counting units (affine_units' count) under the shifted
        geometry.  A candidate out of range under any of its 64 shifts has zeros throughout.  ``units=False`` skips the counts
        (None is returned for them).  offmark.resync.best_shifted_geometry reads the result."""
        t = self.torch
        n, h, w = self._check_frames(frames, t.uint8)
        cands, K = self._cands(cands, 6)
        scores = self._soft(scores, K, 64, copies=n)
        units = None if units is False else self._soft(units, K, 64)
        _hip.check(self.lib.ofmk_svd_affine_phase_scores_rgb8(frames.data_ptr(), n, h, w, int(canvas_hw[0]), int(canvas_hw[1]), cands.data_ptr(),
                                                              K, _hip.scales3(scale, scales), int(blk), scores.data_ptr(), _hip.ptr(units),
                                                              _hip.current_stream(), self._o()))
        return scores, units

    def svd_detect_soft_affine(self, frames, canvas_hw, geom, L, scale=15, scales=None, blk=4, soft=None):
        """svd_detect_soft_warp under an affine ``geom``: the counting units only, unit (i, j) at (i * (W // 8) + j) % L.
        int64 [n, L]; equals warp_affine + svd_detect_soft restricted to the counting units."""
        t = self.torch
        n, h, w = self._check_frames(frames, t.uint8)
        soft = self._soft(soft, n, L)
        g = self._affine_geom(geom)
        _hip.check(self.lib.ofmk_svd_detect_soft_affine_rgb8(frames.data_ptr(), n, h, w, int(canvas_hw[0]), int(canvas_hw[1]), C.byref(g),
                                                             int(L), _hip.scales3(scale, scales), int(blk), soft.data_ptr(),
                                                             _hip.current_stream(), self._o()))
        return soft

    # -- leaks read against their source frames: the sums of a registration step (build extension; offmark.resync.register_leak) --
    def align_sums(self, sources, frames, cands, sums=None):
        """The 29 Gauss-Newton sums of every leak frame warped by every candidate against its source frame (include/offmark_hip.h:
        ofmk_align_sums_rgb8).  sources: uint8 [n, H, W, 3], H, W <= 4096; frames: uint8 [n, h, w, 3]; ``cands``: int64 [K, 6], a
        tensor on this device or an array (copied there) -> int64 [n, K, 29]; a candidate out of range has 29 zeros.  No warped
        frame is written."""
        t = self.torch
        n, H, W = self._check_frames(sources, t.uint8)
        m, h, w = self._check_frames(frames, t.uint8)
        if m != n:
            raise ValueError("one source frame per leak frame")
        cands, K = self._cands(cands, 6)
        sums = self._soft(sums, K, 29, copies=n)
        _hip.check(self.lib.ofmk_align_sums_rgb8(sources.data_ptr(), frames.data_ptr(), n, h, w, H, W, cands.data_ptr(), K, sums.data_ptr(),
                                                 _hip.current_stream(), self._o()))
        return sums

    def halve(self, frames, out=None):
        """The 2x2 box of the registration pyramid: uint8 [n, h, w, 3] -> uint8 [n, h // 2, w // 2, 3], (a + b + c + d + 2) >> 2 per
        channel; an odd last row or column is dropped; both halved sides must be at least 8."""
        t = self.torch
        n, h, w = self._check_frames(frames, t.uint8)
        out = self._out(out, frames, (n, h // 2, w // 2, 3))
        _hip.check(self.lib.ofmk_halve_rgb8(frames.data_ptr(), n, h, w, out.data_ptr(), _hip.current_stream(), self._o()))
        return out

    # -- a leaked clip's frames matched to the source video's (build extension; offmark.temporal) -------------------------------------
    def signatures(self, frames, out=None):
        """The 8 x 8 luma thumbnail of every frame: uint8 [n, h, w, 3], h, w >= 8 -> uint8 [n, 64], cell (i, j) at 8 * i + j, the
        rounded mean of Y = (R + 2 G + B + 2) >> 2 over rows (i h) >> 3 .. ((i + 1) h) >> 3 - 1 and columns likewise
        (include/offmark_hip.h: ofmk_signature_rgb8)."""
        t = self.torch
        n, h, w = self._check_frames(frames, t.uint8)
        out = self._buffer("out", out, (n, 64), t.uint8, self.device)
        _hip.check(self.lib.ofmk_signature_rgb8(frames.data_ptr(), n, h, w, out.data_ptr(), _hip.current_stream(), self._o()))
        return out

    def _signature_list(self, name, s):
        t = self.torch
        if not (isinstance(s, t.Tensor) and s.is_cuda and s.dtype == t.uint8 and s.dim() == 2 and s.shape[1] == 64 and s.shape[0] >= 1
                and s.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous CUDA uint8 tensor [k, 64] with k >= 1")
        return int(s.shape[0])

    def signature_distances(self, a, b, out=None):
        """The L1 distances between two signature lists: uint8 [m, 64] and uint8 [N, 64] -> int32 [m, N], at most 16320
        (ofmk_signature_distances)."""
        m, N = self._signature_list("a", a), self._signature_list("b", b)
        out = self._buffer("out", out, (m, N), self.torch.int32, self.device)
        _hip.check(self.lib.ofmk_signature_distances(a.data_ptr(), m, b.data_ptr(), N, out.data_ptr(), _hip.current_stream(), self._o()))
        return out

    def _window_sums(self, call, words, library, frames, first, span, geom, out):
        """align_residuals / align_moments: int64 [m, span, words] of every leak frame against library[first[i] + j], j < span."""
        t = self.torch
        N, H, W = self._check_frames(library, t.uint8)
        m, h, w = self._check_frames(frames, t.uint8)
        first = self._on_device(first, "int32")
        if first.dim() != 1 or first.shape[0] != m:
            raise ValueError("first must be int32 [m], one entry per leak frame")
        span = int(span)
        if not 1 <= span <= 16:
            raise ValueError("span must be in 1..16")
        out = self._soft(out, span, words, copies=m)
        g = self._affine_geom(geom)
        _hip.check(call(library.data_ptr(), N, frames.data_ptr(), m, h, w, H, W, first.data_ptr(), span, C.byref(g), out.data_ptr(),
                        _hip.current_stream(), self._o()))
        return out

    def align_residuals(self, library, frames, first, span, geom, out=None):
        """The luma residual of every leak frame against a window of source frames under ONE geometry: library uint8 [N, H, W, 3],
        H, W <= 4096; frames uint8 [m, h, w, 3]; ``first``: int32 [m], a tensor on this device or an array (copied there); span in
        1..16 -> int64 [m, span, 2]: entry j of frame i is (sum e^2, contributing pixels) against library[first[i] + j], exactly
        align_sums' [27] and [28] of that pair; (0, 0) where the index leaves the library (ofmk_align_residuals_rgb8).  No warped frame
        and no gathered source is written."""
        return self._window_sums(self.lib.ofmk_align_residuals_rgb8, 2, library, frames, first, span, geom, out)

    # -- a leaked clip whose tone changed as well (build extension; offmark.temporal.read_toned_leak_clip) ----------------------------
    def align_moments(self, library, frames, first, span, geom, out=None):
        """align_residuals' arguments -> int64 [m, span, 6]: entry j of frame i is (count, sum l, sum s, sum l^2, sum s^2, sum l s)
        over align_residuals' contributing pixels, l the warped luma of leak frame i, s the luma of library[first[i] + j]; six zeros
        where the index leaves the library (ofmk_align_moments_rgb8).  [3] + [4] - 2 [5] is align_residuals' sum e^2, [0] its count."""
        return self._window_sums(self.lib.ofmk_align_moments_rgb8, 6, library, frames, first, span, geom, out)

    def signature_ranks(self, sig, out=None):
        """The rank signature: uint8 [n, 64] -> uint8 [n, 64], rank[f, c] = #{c' : (sig[f, c'], c') < (sig[f, c], c)}, a permutation
        of 0..63 that an increasing tone curve leaves unchanged (ofmk_signature_ranks)."""
        n = self._signature_list("sig", sig)
        out = self._buffer("out", out, (n, 64), self.torch.uint8, self.device)
        _hip.check(self.lib.ofmk_signature_ranks(sig.data_ptr(), n, out.data_ptr(), _hip.current_stream(), self._o()))
        return out

    # -- leaks whose values changed: a tone curve fitted against the source frames (build extension; offmark.tone) ---------------------
    def histograms(self, frames, out=None):
        """The per-channel histograms of every frame: uint8 [n, h, w, 3] -> int64 [n, 3, 256], entry [f, c, v] the number of pixels of
        frame f whose channel c equals v (include/offmark_hip.h: ofmk_histograms_rgb8)."""
        t = self.torch
        n, h, w = self._check_frames(frames, t.uint8)
        out = self._soft(out, 3, 256, copies=n)
        _hip.check(self.lib.ofmk_histograms_rgb8(frames.data_ptr(), n, h, w, out.data_ptr(), _hip.current_stream(), self._o()))
        return out

    def tone_sums(self, sources, frames, cands, sums=None):
        """Per leak value, how many canvas pixels show it and what the source holds there (ofmk_tone_sums_rgb8).  sources: uint8
        [n, H, W, 3], H, W <= 4096; frames: uint8 [n, h, w, 3]; ``cands``: int64 [K, 6], a tensor on this device or an array (copied
        there) -> int64 [n, K, 3, 256, 2]: entry [f, k, c, v] is (count, sum of the source's channel c) over the canvas pixels inside
        the leak where frame f warped by candidate k has v in channel c; a candidate out of range has zeros.  No warped frame is
        written."""
        t = self.torch
        n, H, W = self._check_frames(sources, t.uint8)
        m, h, w = self._check_frames(frames, t.uint8)
        if m != n:
            raise ValueError("one source frame per leak frame")
        cands, K = self._cands(cands, 6)
        sums = self._buffer("sums", sums, (n, K, 3, 256, 2), t.int64, self.device)
        _hip.check(self.lib.ofmk_tone_sums_rgb8(sources.data_ptr(), frames.data_ptr(), n, h, w, H, W, cands.data_ptr(), K, sums.data_ptr(),
                                                _hip.current_stream(), self._o()))
        return sums

    def apply_tone(self, frames, lut, out=None):
        """out[f, y, x, c] = lut[c, frames[f, y, x, c]]: uint8 [n, h, w, 3] -> uint8 [n, h, w, 3]; ``lut``: uint8 [3, 256], a tensor on
        this device or an array (copied there); ``out`` may be ``frames`` itself (ofmk_apply_tone_rgb8)."""
        t = self.torch
        n, h, w = self._check_frames(frames, t.uint8)
        lut = self._on_device(lut, "uint8")
        if tuple(lut.shape) != (3, 256):
            raise ValueError("lut must be uint8 [3, 256]")
        out = self._out(out, frames)
        _hip.check(self.lib.ofmk_apply_tone_rgb8(frames.data_ptr(), n, h, w, lut.data_ptr(), out.data_ptr(), _hip.current_stream(), self._o()))
        return out

    # -- leaks whose colours changed: a matrix fitted against the source frames (build extension; offmark.colour) ----------------------
    def colour_sums(self, sources, frames, cands, sums=None):
        """The 28 least-squares sums of source ~ M leak + t per frame and candidate (ofmk_colour_sums_rgb8).  sources: uint8
        [n, H, W, 3], H, W <= 4096; frames: uint8 [n, h, w, 3]; ``cands``: int64 [K, 6], a tensor on this device or an array (copied
        there) -> int64 [n, K, 28] over the canvas pixels inside the leak whose three warped bytes l all lie in 1..254, s the source's
        bytes there: [0] the count, [1..3] sum l, [4..6] sum s, [7..12] sum l_i l_j and [13..18] sum s_i s_j for (i, j) = 00 01 02 11
        12 22, [19 + 3 i + j] sum l_i s_j; a candidate out of range has zeros.  No warped frame is written."""
        t = self.torch
        n, H, W = self._check_frames(sources, t.uint8)
        m, h, w = self._check_frames(frames, t.uint8)
        if m != n:
            raise ValueError("one source frame per leak frame")
        cands, K = self._cands(cands, 6)
        sums = self._buffer("sums", sums, (n, K, 28), t.int64, self.device)
        _hip.check(self.lib.ofmk_colour_sums_rgb8(sources.data_ptr(), frames.data_ptr(), n, h, w, H, W, cands.data_ptr(), K, sums.data_ptr(),
                                                  _hip.current_stream(), self._o()))
        return sums

    def apply_colour(self, frames, matrix, out=None):
        """out[.., c] = clip((m[c, 0] r + m[c, 1] g + m[c, 2] b + m[c, 3] + 32768) >> 16, 0, 255) per pixel: uint8 [n, h, w, 3] -> uint8
        [n, h, w, 3]; ``matrix``: integers [3, 4] in Q16 on the HOST, |coefficient| <= 2^21 and |offset| <= 2^28 (else ValueError);
        ``out`` may be ``frames`` itself (ofmk_apply_colour_rgb8)."""
        t = self.torch
        n, h, w = self._check_frames(frames, t.uint8)
        m = np.asarray(matrix.cpu() if isinstance(matrix, t.Tensor) else matrix)
        if m.shape != (3, 4) or m.dtype.kind not in "iu":
            raise ValueError("matrix must be integers of shape [3, 4]")
        if (np.abs(m[:, :3].astype(np.int64)) > 1 << 21).any() or (np.abs(m[:, 3].astype(np.int64)) > 1 << 28).any():
            raise ValueError("matrix: |coefficient| <= 2^21 and |offset| <= 2^28")
        m = np.ascontiguousarray(m, dtype=np.int32)
        out = self._out(out, frames)
        _hip.check(self.lib.ofmk_apply_colour_rgb8(frames.data_ptr(), n, h, w, m.ctypes.data_as(C.POINTER(C.c_int32)), out.data_ptr(),
                                                   _hip.current_stream(), self._o()))
        return out

    def svd_embed_detect(self, frames, wm, L, scale=15, wm_row=None, out=None, want_bits=False, scales=None, blk=4, counts=None,
                         partial=False):
        t = self.torch
        n, H, W = self._check_frames(frames, t.uint8)
        wm = self._wm(wm, H * W // 64)
        rows = self._rows(wm_row, n, wm.shape[0])
        out = self._out(out, frames)
        counts, flag = self._svd_counts(counts, n, H, W, L, blk, partial)
        bits = t.empty((n, self.svd_bits_per_frame(H, W, blk)), dtype=t.uint8, device=self.device) if want_bits else None
        _hip.check(self.lib.ofmk_svd_embed_detect_rgb8(frames.data_ptr(), out.data_ptr(), n, H, W, wm.data_ptr(),
                                                       wm.shape[0], _hip.ptr(rows), _hip.scales3(scale, scales), int(blk), int(L),
                                                       counts.data_ptr(), _hip.ptr(bits), _hip.current_stream(),
                                                       self._o(extra_flags=flag)))
        return out, counts, bits

    # -- C marked copies of the same frames in one pass (the A/B workflow) ----------------------------------------------
    _MAX_COPIES = 16              # a payload's copy field has 4 bits (fingerprint.payload_for_segment)

    def _copy_rows(self, wm_rows, n, n_wm, copies=None):
        """Watermark rows of the copies -> (device int32 [C, n] or None, C).  ``wm_rows`` None: copy c uses row c, C =
        ``copies`` (default: every row of the table).  Host arrays are range-checked as _rows checks them; device tensors when
        ``debug_checks`` is set (the kernels clamp every entry into [0, n_wm) either way)."""
        t = self.torch
        if wm_rows is None:
            C = n_wm if copies is None else int(copies)
        else:
            if isinstance(wm_rows, (list, tuple)):
                wm_rows = np.asarray(wm_rows)
            if wm_rows.ndim != 2 or wm_rows.shape[1] != n or (copies is not None and wm_rows.shape[0] != copies):
                raise ValueError(f"wm_rows must be [copies, {n}] (one row per frame and copy); got {tuple(wm_rows.shape)}")
            C = int(wm_rows.shape[0])
            if isinstance(wm_rows, np.ndarray):
                if wm_rows.size and (wm_rows.min() < 0 or wm_rows.max() >= n_wm):
                    raise ValueError(f"wm_rows entries must be in [0, {n_wm}); got [{wm_rows.min()}, {wm_rows.max()}]")
                wm_rows = t.from_numpy(np.ascontiguousarray(wm_rows).astype(np.int32))
            elif (not wm_rows.is_cuda or self.debug_checks) and wm_rows.numel() and (
                    int(wm_rows.min()) < 0 or int(wm_rows.max()) >= n_wm):
                raise ValueError(f"wm_rows entries must be in [0, {n_wm}); got [{int(wm_rows.min())}, {int(wm_rows.max())}]")
            wm_rows = wm_rows.to(device=self.device, dtype=t.int32).contiguous()
        if not 1 <= C <= self._MAX_COPIES:
            raise ValueError(f"copies must be in [1, {self._MAX_COPIES}]; got {C}")
        return wm_rows, C

    def embed_copies(self, frames, wm, wm_rows, alpha=20, out=None, copies=None):
        """C differently marked copies of the same frames in one pass: uint8 [C, n, H, W, 3] whose copy c equals, byte for byte,
        ``embed(frames, wm, alpha, wm_row=wm_rows[c])``.  wm_rows: [C, n] rows of ``wm`` per copy and frame, or None (copy c uses
        row c; C = ``copies``, default the number of rows).  The analysis of the frames is done once for all copies."""
        t = self.torch
        n, H, W = self._check_frames(frames, t.uint8)
        wm = self._wm(wm, H * W // 64)
        rows, C = self._copy_rows(wm_rows, n, wm.shape[0], copies)
        out = self._out(out, frames, (C, n, H, W, 3))
        cf = self._chunk(n, H, W)
        ws = self.workspace(H, W, cf)
        _hip.check(self.lib.ofmk_embed_copies_rgb8(frames.data_ptr(), out.data_ptr(), C, n, H, W, wm.data_ptr(), wm.shape[0],
                                                   _hip.ptr(rows), float(alpha), cf, ws.data_ptr(), ws.numel(), _hip.current_stream(),
                                                   self._o(min(cf, n) * H * W * 3)))
        return out

    def embed_detect_copies(self, frames, wm, wm_rows, L, alpha=20, out=None, want_bits=False, counts=None, copies=None, soft=None):
        """embed_copies and the verify of every copy in the same pass: returns (out uint8 [C, n, H, W, 3], counts int32 [C, n, L],
        bits uint8 [C, n, N] or None).  ``out`` is embed_copies' result byte for byte; counts[c] / bits[c] are what
        ``embed_detect(frames, wm, L, alpha, wm_row=wm_rows[c])`` returns, i.e. ``detect(out[c], L, alpha)``.  Each copy is read out
        from the pixels the mark kernel still holds, so no copy is read back (csrc/copies_kernels.hiph).
        ``soft`` (build extension): True or an int64 [C, n, L] tensor -- also the soft sums of every copy, soft[c] ==
        ``detect_soft(out[c], L, alpha)``, from the same records; returned as a fourth element."""
        t = self.torch
        n, H, W = self._check_frames(frames, t.uint8)
        N = H * W // 64
        wm = self._wm(wm, N)
        rows, C = self._copy_rows(wm_rows, n, wm.shape[0], copies)
        out = self._out(out, frames, (C, n, H, W, 3))
        L = int(L)
        counts = self._counts(counts, n, L, copies=C)
        bits = t.empty((C, n, N), dtype=t.uint8, device=self.device) if want_bits else None
        cf = self._chunk(n, H, W)
        ws = self.copies_workspace(H, W, cf, C)
        stream = _hip.current_stream()
        o = self._o(min(cf, n) * H * W * 3)
        if soft is None or soft is False:
            _hip.check(self.lib.ofmk_embed_detect_copies_rgb8(frames.data_ptr(), out.data_ptr(), C, n, H, W, wm.data_ptr(),
                                                              wm.shape[0], _hip.ptr(rows), float(alpha), L, counts.data_ptr(),
                                                              _hip.ptr(bits), cf, ws.data_ptr(), ws.numel(), stream, o))
            return out, counts, bits
        soft = self._soft(soft, n, L, copies=C)
        _hip.check(self.lib.ofmk_embed_detect_copies_soft_rgb8(frames.data_ptr(), out.data_ptr(), C, n, H, W, wm.data_ptr(),
                                                               wm.shape[0], _hip.ptr(rows), float(alpha), L, counts.data_ptr(),
                                                               _hip.ptr(bits), soft.data_ptr(), cf, ws.data_ptr(), ws.numel(),
                                                               stream, o))
        return out, counts, bits, soft

    def svd_embed_copies(self, frames, wm, wm_rows, scale=15, scales=None, blk=4, out=None, L=None, want_bits=False, counts=None,
                         partial=False, copies=None, soft=None):
        """The DwtDctSvd codec's copies in one pass: copy c of the uint8 [C, n, H, W, 3] result equals ``svd_embed`` with
        ``wm_row=wm_rows[c]``.  With ``L``: also the verify of every copy, returns (out, counts [C, n, L] -- or, ``partial``,
        [C, n, tiles, L] -- and bits [C, n, bits_per_frame] or None), each copy's equal to ``svd_embed_detect``'s.
        ``soft`` (build extension, needs ``L``): True or an int64 [C, n, L] tensor -- also the soft sums of every copy, soft[c] ==
        ``svd_detect_soft(out[c], L, ...)``, from the pixels the kernel still holds (blk 4); returned as a fourth element."""
        t = self.torch
        n, H, W = self._check_frames(frames, t.uint8)
        wm = self._wm(wm, H * W // 64)
        rows, C = self._copy_rows(wm_rows, n, wm.shape[0], copies)
        out = self._out(out, frames, (C, n, H, W, 3))
        flag, bits = 0, None
        if L is not None:
            counts, flag = self._svd_counts(counts, n, H, W, L, blk, partial, copies=C)
            if want_bits:
                bits = t.empty((C, n, self.svd_bits_per_frame(H, W, blk)), dtype=t.uint8, device=self.device)
        if soft is not None and soft is not False:
            if L is None:
                raise ValueError("soft needs the payload length L")
            soft = self._soft(soft, n, int(L), copies=C)
            _hip.check(self.lib.ofmk_svd_embed_copies_soft_rgb8(frames.data_ptr(), out.data_ptr(), C, n, H, W, wm.data_ptr(), wm.shape[0],
                                                                _hip.ptr(rows), _hip.scales3(scale, scales), int(blk), int(L),
                                                                _hip.ptr(counts), _hip.ptr(bits), soft.data_ptr(), _hip.current_stream(),
                                                                self._o(extra_flags=flag)))
            return out, counts, bits, soft
        _hip.check(self.lib.ofmk_svd_embed_copies_rgb8(frames.data_ptr(), out.data_ptr(), C, n, H, W, wm.data_ptr(), wm.shape[0],
                                                       _hip.ptr(rows), _hip.scales3(scale, scales), int(blk),
                                                       int(L) if L is not None else 0, _hip.ptr(counts) if L is not None else None,
                                                       _hip.ptr(bits), _hip.current_stream(), self._o(extra_flags=flag)))
        return out if L is None else (out, counts, bits)

    # -- DwtDctSvd codec on planar 8-bit YUV 4:2:0 (one tile-local pass, the conversions fused in) -------------------
    def svd_embed_yuv420(self, planes, H, W, wm, scale=15, wm_row=None, out=None, scales=None, blk=4, layout="i420"):
        """Mark frames given as 4:2:0 planes [n, 1.5*H*W]; returns marked planes of the same layout.  Equal, bit for bit, to
        rgb_to_yuv420(svd_embed(yuv420_to_rgb(planes))), blk = 8's uncovered fringe included (its 4:2:0 round trip)."""
        n = self._check_planar(planes, H, W)
        wm = self._wm(wm, H * W // 64)
        rows = self._rows(wm_row, n, wm.shape[0])
        out = self._out(out, planes)
        _hip.check(self.lib.ofmk_svd_embed_yuv420(planes.data_ptr(), out.data_ptr(), self._layout(layout), n, H, W, wm.data_ptr(),
                                                  wm.shape[0], _hip.ptr(rows), _hip.scales3(scale, scales), int(blk),
                                                  _hip.current_stream(), self._o()))
        return out

    def svd_detect_yuv420(self, planes, H, W, L, scale=15, want_bits=False, scales=None, blk=4, counts=None, partial=False,
                          layout="i420"):
        """Read-out of 4:2:0 planes: equal to svd_detect(yuv420_to_rgb(planes)).  Returns (counts, bits or None)."""
        t = self.torch
        n = self._check_planar(planes, H, W)
        counts, flag = self._svd_counts(counts, n, H, W, L, blk, partial)
        bits = t.empty((n, self.svd_bits_per_frame(H, W, blk)), dtype=t.uint8, device=self.device) if want_bits else None
        _hip.check(self.lib.ofmk_svd_detect_yuv420(planes.data_ptr(), self._layout(layout), n, H, W, int(L), _hip.scales3(scale, scales),
                                                   int(blk), counts.data_ptr(), _hip.ptr(bits), _hip.current_stream(),
                                                   self._o(extra_flags=flag)))
        return counts, bits

    def svd_detect_soft_yuv420(self, planes, H, W, L, scale=15, scales=None, blk=4, layout="i420", soft=None):
        """Build extension (not reference semantics): svd_detect_soft on 4:2:0 planes, int64 [n, L]; equal, integer for integer,
        to svd_detect_soft(yuv420_to_rgb(planes))."""
        n = self._check_planar(planes, H, W)
        soft = self._soft(soft, n, L)
        _hip.check(self.lib.ofmk_svd_detect_soft_yuv420(planes.data_ptr(), self._layout(layout), n, H, W, int(L),
                                                        _hip.scales3(scale, scales), int(blk), soft.data_ptr(), _hip.current_stream(),
                                                        self._o()))
        return soft

    # -- block-grid resync of cropped 4:2:0 planes (build extension, not reference semantics; blk 4, channel 1; offmark.resync) --
    # Only the 16 phases with even py and px exist on planes: an odd crop offset would need chroma resampled by half a sample,
    # which destroys a chroma mark (include/offmark_hip.h).  H and W need only be even and >= 8.
    def _check_planar_even(self, planes, H, W):
        t = self.torch
        if H < 8 or W < 8 or H % 2 or W % 2:
            raise ValueError("cropped 4:2:0 frames need even H and W of at least 8")
        if not (isinstance(planes, t.Tensor) and planes.is_cuda and planes.dtype == t.uint8 and planes.dim() == 2
                and planes.shape[1] == H * W * 3 // 2 and planes.is_contiguous()):
            raise ValueError("planes must be a contiguous CUDA uint8 tensor [n, H*W*3/2] (I420: Y|U|V, NV12: Y|UV per frame)")
        return planes.shape[0]

    def svd_sync_scores_yuv420(self, planes, H, W, scale=15, scales=None, blk=4, layout="i420", scores=None):
        """The dense phase search on planes: int64 [n, 64].  For even py and px, entry 8 * py + px = the sum of |unit metric| of
        svd_detect_soft_yuv420 (blk 4) over the units of the frame's sub-planes for the pixel window [py:py + 8r, px:px + 8c],
        r = (H - py) // 8, c = (W - px) // 8 -- the even entries of svd_sync_scores(yuv420_to_rgb(planes)), integer for integer.
        Odd phases and phases without a unit are 0.  offmark.resync.best_phase(..., even_only=True) reads it."""
        return self._svd_sync_scores(self._planar_leak(planes, H, W, layout), scale, scales, blk, scores)

    def svd_detect_soft_window_yuv420(self, planes, H, W, L, phase, canvas_cols, base=0, scale=15, scales=None, blk=4, layout="i420",
                                      soft=None):
        """svd_detect_soft_yuv420 of the units at the even grid ``phase`` = (py, px): unit (i, j) is the 8x8 block at pixel
        (py + 8i, px + 8j), read through the frame's own pitch, and adds into position (base + i * canvas_cols + j) % L.
        int64 [n, L]."""
        return self._svd_detect_soft_window(self._planar_leak(planes, H, W, layout), L, phase, canvas_cols, base, scale, scales, blk, soft)

    def sync_workspace_yuv420(self, H: int, W: int, frames: int):
        """Scratch of sync_scores_yuv420 for `frames` frames in flight (ofmk_sync_workspace_bytes_yuv420: one record per even
        pixel origin).  A cache of its own, as sync_workspace()."""
        return self._sync_ws("sync420", self.lib.ofmk_sync_workspace_bytes_yuv420, H, W, frames)

    def sync_scores_yuv420(self, planes, H, W, alpha=20, layout="i420", scores=None):
        """The DCT codec's dense phase search on planes: int64 [n, 64].  For even py and px, entry 8 * py + px =
        ``detect_soft_yuv420(sub, blocks, alpha).abs().sum(1)`` of the frame's sub-planes for the pixel window [py:py + 8r,
        px:px + 8c] -- masks and frame mean taken from that sub-frame -- integer for integer, which is also that entry of
        sync_scores(yuv420_to_rgb(planes)).  Odd phases and phases without a block are 0."""
        # 3 bytes of records per pixel against 1.5 of planes: half the frame budget keeps the records at the frames' size
        return self._sync_scores(self._planar_leak(planes, H, W, layout), 2, self.sync_workspace_yuv420, alpha, scores)

    def detect_soft_window_yuv420(self, planes, H, W, L, phase, canvas_cols, base=0, alpha=20, layout="i420", soft=None):
        """detect_soft_yuv420 of the blocks at the even grid ``phase`` = (py, px): block (i, j) is the 8x8 block at pixel
        (py + 8i, px + 8j), read through the frame's own pitch, and adds into position (base + i * canvas_cols + j) % L.  Masks
        and frame mean come from the window.  int64 [n, L]."""
        return self._detect_soft_window(self._planar_leak(planes, H, W, layout), "window420", L, phase, canvas_cols, base, alpha, soft)

    def svd_embed_detect_yuv420(self, planes, H, W, wm, L, scale=15, wm_row=None, out=None, want_bits=False, scales=None, blk=4,
                                counts=None, partial=False, layout="i420"):
        """Mark and verify on planes; counts / bits are what a reader of the WRITTEN planes gets (== svd_detect_yuv420(out))."""
        t = self.torch
        n = self._check_planar(planes, H, W)
        wm = self._wm(wm, H * W // 64)
        rows = self._rows(wm_row, n, wm.shape[0])
        out = self._out(out, planes)
        counts, flag = self._svd_counts(counts, n, H, W, L, blk, partial)
        bits = t.empty((n, self.svd_bits_per_frame(H, W, blk)), dtype=t.uint8, device=self.device) if want_bits else None
        _hip.check(self.lib.ofmk_svd_embed_detect_yuv420(planes.data_ptr(), out.data_ptr(), self._layout(layout), n, H, W, wm.data_ptr(),
                                                         wm.shape[0], _hip.ptr(rows), _hip.scales3(scale, scales), int(blk), int(L),
                                                         counts.data_ptr(), _hip.ptr(bits), _hip.current_stream(),
                                                         self._o(extra_flags=flag)))
        return out, counts, bits

    # -- C marked copies of the same 4:2:0 frames in one pass (csrc/planar_copies_kernels.hiph) ------------------------------
    def embed_copies_yuv420(self, planes, H, W, wm, wm_rows, alpha=20, out=None, copies=None, layout="i420"):
        """C differently marked copies of frames given as 4:2:0 planes [n, 1.5*H*W] in one pass: uint8 [C, n, 1.5*H*W] of the same
        layout whose copy c equals, byte for byte, ``embed_yuv420(planes, H, W, wm, alpha, wm_row=wm_rows[c])``.  wm_rows as
        embed_copies.  The frames are analyzed and converted once for all copies."""
        n = self._check_planar(planes, H, W)
        fmt = self._layout(layout)
        wm = self._wm(wm, H * W // 64)
        rows, C = self._copy_rows(wm_rows, n, wm.shape[0], copies)
        out = self._out(out, planes, (C, n, H * W * 3 // 2))
        cf = self._chunk(n, H, W)
        ws = self.workspace(H, W, cf)
        _hip.check(self.lib.ofmk_embed_copies_yuv420(planes.data_ptr(), out.data_ptr(), fmt, C, n, H, W, wm.data_ptr(), wm.shape[0],
                                                     _hip.ptr(rows), float(alpha), cf, ws.data_ptr(), ws.numel(),
                                                     _hip.current_stream(), self._o()))
        return out

    def embed_detect_copies_yuv420(self, planes, H, W, wm, wm_rows, L, alpha=20, out=None, want_bits=False, counts=None, copies=None,
                                   layout="i420", soft=None):
        """embed_copies_yuv420 and the verify of every copy in the same pass: returns (out uint8 [C, n, 1.5*H*W], counts int32
        [C, n, L], bits uint8 [C, n, N] or None).  ``out`` is embed_copies_yuv420's result byte for byte; counts[c] / bits[c] are what
        ``embed_detect_yuv420(planes, H, W, wm, L, alpha, wm_row=wm_rows[c])`` returns, i.e. ``detect_yuv420(out[c], H, W, L, alpha)``.
        Each copy is read out from the pixels the mark kernel still holds, so no copy is read back; the kernel runs the fused
        mark + verify body once per marked form a block needs (at most two), not once per copy (csrc/planar_copies_kernels.hiph).
        ``soft`` (build extension): True or an int64 [C, n, L] tensor -- also the soft sums of every copy, soft[c] ==
        ``detect_soft_yuv420(out[c], H, W, L, alpha)``, from the same records; returned as a fourth element."""
        t = self.torch
        n = self._check_planar(planes, H, W)
        fmt = self._layout(layout)
        N = H * W // 64
        wm = self._wm(wm, N)
        rows, C = self._copy_rows(wm_rows, n, wm.shape[0], copies)
        out = self._out(out, planes, (C, n, H * W * 3 // 2))
        L = int(L)
        counts = self._counts(counts, n, L, copies=C)
        bits = t.empty((C, n, N), dtype=t.uint8, device=self.device) if want_bits else None
        want_soft = soft is not None and soft is not False
        if want_soft:
            soft = self._soft(soft, n, L, copies=C)
        cf = self._chunk(n, H, W)
        ws = self.copies_workspace(H, W, cf, C)
        if want_soft:
            _hip.check(self.lib.ofmk_embed_detect_copies_soft_yuv420(planes.data_ptr(), out.data_ptr(), fmt, C, n, H, W, wm.data_ptr(),
                                                                     wm.shape[0], _hip.ptr(rows), float(alpha), L, counts.data_ptr(),
                                                                     _hip.ptr(bits), soft.data_ptr(), cf, ws.data_ptr(), ws.numel(),
                                                                     _hip.current_stream(), self._o()))
            return out, counts, bits, soft
        _hip.check(self.lib.ofmk_embed_detect_copies_yuv420(planes.data_ptr(), out.data_ptr(), fmt, C, n, H, W, wm.data_ptr(),
                                                            wm.shape[0], _hip.ptr(rows), float(alpha), L, counts.data_ptr(),
                                                            _hip.ptr(bits), cf, ws.data_ptr(), ws.numel(), _hip.current_stream(),
                                                            self._o()))
        return out, counts, bits

    def svd_embed_copies_yuv420(self, planes, H, W, wm, wm_rows, scale=15, scales=None, blk=4, out=None, L=None, want_bits=False,
                                counts=None, partial=False, copies=None, layout="i420", soft=None):
        """The DwtDctSvd codec's copies on 4:2:0 planes in one pass: copy c of the uint8 [C, n, 1.5*H*W] result equals
        ``svd_embed_yuv420`` with ``wm_row=wm_rows[c]``.  With ``L``: also the verify of every copy, returns (out, counts [C, n, L]
        -- or, ``partial``, [C, n, tiles, L] -- and bits [C, n, bits_per_frame] or None), each copy's equal to
        ``svd_embed_detect_yuv420``'s.  ``soft`` (build extension, needs ``L``): True or an int64 [C, n, L] tensor -- also soft[c] ==
        ``svd_detect_soft_yuv420(out[c], ...)``, returned as a fourth element."""
        t = self.torch
        n = self._check_planar(planes, H, W)
        fmt = self._layout(layout)
        wm = self._wm(wm, H * W // 64)
        rows, C = self._copy_rows(wm_rows, n, wm.shape[0], copies)
        out = self._out(out, planes, (C, n, H * W * 3 // 2))
        flag, bits = 0, None
        if L is not None:
            counts, flag = self._svd_counts(counts, n, H, W, L, blk, partial, copies=C)
            if want_bits:
                bits = t.empty((C, n, self.svd_bits_per_frame(H, W, blk)), dtype=t.uint8, device=self.device)
        if soft is not None and soft is not False:
            if L is None:
                raise ValueError("soft needs the payload length L")
            soft = self._soft(soft, n, int(L), copies=C)
            _hip.check(self.lib.ofmk_svd_embed_copies_soft_yuv420(planes.data_ptr(), out.data_ptr(), fmt, C, n, H, W, wm.data_ptr(),
                                                                  wm.shape[0], _hip.ptr(rows), _hip.scales3(scale, scales), int(blk), int(L),
                                                                  _hip.ptr(counts), _hip.ptr(bits), soft.data_ptr(),
                                                                  _hip.current_stream(), self._o(extra_flags=flag)))
            return out, counts, bits, soft
        _hip.check(self.lib.ofmk_svd_embed_copies_yuv420(planes.data_ptr(), out.data_ptr(), fmt, C, n, H, W, wm.data_ptr(),
                                                         wm.shape[0], _hip.ptr(rows), _hip.scales3(scale, scales), int(blk),
                                                         int(L) if L is not None else 0, _hip.ptr(counts) if L is not None else None,
                                                         _hip.ptr(bits), _hip.current_stream(), self._o(extra_flags=flag)))
        return out if L is None else (out, counts, bits)

    def svd_encode_yuv(self, yuv, wm, scale=15, scales=None, blk=4):
        t = self.torch
        n, H, W = self._check_frames(yuv, t.float32)
        wm = self._wm(wm, H * W // 64)
        _hip.check(self.lib.ofmk_svd_encode_yuv32f(yuv.data_ptr(), n, H, W, wm.data_ptr(), wm.shape[0], None,
                                                   _hip.scales3(scale, scales), int(blk), _hip.current_stream(), self._o()))
        return yuv

    def svd_decode_yuv(self, yuv, scale=15, scales=None, blk=4):
        t = self.torch
        n, H, W = self._check_frames(yuv, t.float32)
        bits = t.empty((n, self.svd_bits_per_frame(H, W, blk)), dtype=t.uint8, device=self.device)
        _hip.check(self.lib.ofmk_svd_decode_yuv32f(yuv.data_ptr(), n, H, W, _hip.scales3(scale, scales), int(blk), bits.data_ptr(),
                                                   _hip.current_stream(), self._o()))
        return bits

    # -- parity planes ----------------------------------------------------------------------------
    def debug_planes(self, frame, alpha=20, wm=None):
        """One frame (u8 [H,W,3] or f32 YUV [H,W,3], CUDA).  Returns a dict of host numpy planes."""
        t = self.torch
        is_yuv = frame.dtype == t.float32
        H, W, _ = frame.shape
        h8, w8 = H // 8, W // 8
        mk = lambda dt: t.empty((h8, w8), dtype=dt, device=self.device)  # noqa: E731
        ydc, c21_pre, c21_post = mk(t.float32), mk(t.float32), mk(t.float32)
        lum, tex, step = mk(t.float64), mk(t.float64), mk(t.float64)
        wmt = self._wm(wm, H * W // 64) if wm is not None else None
        ws = self.workspace(H, W, 1)
        _hip.check(self.lib.ofmk_debug_planes(frame.contiguous().data_ptr(), int(is_yuv), H, W, float(alpha),
                                              _hip.ptr(wmt), ydc.data_ptr(), lum.data_ptr(), tex.data_ptr(),
                                              step.data_ptr(), c21_pre.data_ptr(),
                                              c21_post.data_ptr() if wmt is not None else None,
                                              ws.data_ptr(), ws.numel(), _hip.current_stream(), self._o()))
        out = dict(y_dc=ydc, lum=lum, tex=tex, step=step, c21_pre=c21_pre)
        if wmt is not None:
            out["c21_post"] = c21_post
        return {k: v.cpu().numpy() for k, v in out.items()}


def payload_means(counts: np.ndarray, N: int, L: int) -> np.ndarray:
    """Host epilogue of DeShuffler.degenerate (de_shuffler.py:17-18): mean of bits[i::L].

    counts[..., i] is the number of ones among the N-long bit vector's entries i, i+L, ...;
    that slice has ceil((N - i) / L) entries (fewer than N/L for the tail when L does not divide N).
    """
    i = np.arange(L)
    lens = np.where(i < N, (N - i + L - 1) // L, 0).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return counts.astype(np.float64) / lens
