/* offmark_hip.h -- C ABI of the MI355X (gfx950) DCT frame-watermark engine.
 *
 * The reference (vikasdimaniya/video-fingerprinting, "offmark") is pure Python and has no FFI
 * of its own; each entry point below names the reference interface it replaces
 * (paths relative to the reference root).  The Python package `offmark` in this repository
 * binds these symbols with ctypes (video-fingerprinting_amd/offmark/_hip.py); INTEGRATION.md
 * shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer marked "device" is HBM memory owned by the caller (e.g. torch tensors);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is only
 *     ENQUEUED on it: no allocation, no host synchronisation, no internal threads, so every
 *     compute call may be captured into a hipGraph (unless it carries an ofmk_timing object);
 *   - re-entrant: the library has NO mutable state besides the calling thread's error text.
 *     Everything a call needs arrives in its arguments; per-call options travel in `ofmk_opts`
 *     (NULL = defaults), the LAST argument of EVERY compute entry point (since ABI 3; only the
 *     bandwidth probes and the timing-object functions at the end of this file take none).  Two host threads may drive two engines (own workspace, own stream,
 *     own timing object) concurrently (tests/test_gpu_parity.py::test_two_threads_two_engines);
 *   - return value 0 = OK, negative = error (OFMK_E_*); ofmk_last_error() gives the text for
 *     the calling thread; nothing throws across this boundary;
 *   - frames are interleaved 8-bit, 3 channels, row-major [n][H][W][3] exactly as
 *     FileDecoder.read() delivers them (src/offmark/video/frame_reader.py:53-64).  Channel 0
 *     is treated as "B" by the colour transform, as the reference does
 *     (src/offmark/video/embedder.py:34).
 *   - one watermark bit per 8x8 pixel block, raster order, N = H*W/64 entries per frame of
 *     which the first (H/8)*(W/8) are used (src/offmark/embed/dct_encoder.py:13-16,25-26).
 */
#ifndef OFFMARK_HIP_H
#define OFFMARK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFMK_ABI_VERSION 6

#define OFMK_OK            0
#define OFMK_E_ARG        -1   /* null pointer / non-positive size / H or W < 8 */
#define OFMK_E_WORKSPACE  -2   /* workspace smaller than ofmk_workspace_bytes(1, H, W) */
#define OFMK_E_HIP        -3   /* a HIP call failed; text in ofmk_last_error() */

int ofmk_version(void);
const char *ofmk_last_error(void);

/* Per-call options (the reference's codecs are stateless objects configured by constructor kwargs,
 * src/offmark/embed/dct_encoder.py:6-16; this is the same idea at the C boundary).  Pass NULL for defaults. */
typedef struct ofmk_timing ofmk_timing;     /* opaque, see ofmk_timing_create */
typedef struct ofmk_opts {
    uint32_t flags;          /* OFMK_F_*; unknown bits are rejected (OFMK_E_ARG) */
    uint32_t xcds;           /* XCDs the XCD-aware tile order assumes: 0 = 8 (MI355X, SPX mode), 1 = linear order, > 64 rejected.
                                ABI 3 called this word `reserved` and required 0 */
    ofmk_timing *timing;     /* NULL = launches carry no events */
} ofmk_opts;
/* ofmk_embed_detect_rgb8: embed, then detect the written frames with the stand-alone detect kernels
 * (analyze runs on the marked frames: 12 B/px of traffic) instead of the fused mark+verify kernel
 * (9 B/px).  Same results bit for bit. */
#define OFMK_F_SEPARATE_DETECT 1u
/* Tile order of the frame-WRITING DCT kernel (ofmk_embed_rgb8, ofmk_embed_detect_rgb8, ofmk_stage_mark_rgb8).  The kernel is
 * one linear grid of 48 KiB tiles; the hardware deals consecutive workgroups round-robin to the XCDs.  XCD-aware order: every XCD walks one contiguous 1/xcds of the launch's frames (tile = (L % xcds) * ceil(G / xcds)
 * + L / xcds); linear order: tile = workgroup index.  A pure permutation of the work: results are identical bit for bit either
 * way.  DEFAULT (neither flag, since ABI 5): a static rule on the launch's size -- XCD-aware when the launch reads at least
 * OFMK_XCD_TILES_MIN_BYTES of frames (192 frames of 1080p), linear below -- which is what interleaved A/B runs on MI355X say
 * (large launches: XCD-aware wins by 1.5-6 % or ties, depending on where the driver placed the caller's frames; 48-96 frames of
 * 1080p: linear wins by 1-4 %; profiles/r4_mark_fused_pass.txt, profiles/r6_mark_ladder.txt).
 * The two flags force an order (a caller that has measured its own box); both at once are rejected.  ABI 4 defaulted to the XCD-aware order at every size.  The read-only and one-pass kernels always run in linear
 * order (measured faster there).  The reference has no counterpart: its loop is one frame at a time
 * (src/offmark/video/embedder.py:18-31). */
#define OFMK_F_LINEAR_TILES 2u
#define OFMK_F_XCD_TILES 4u
#define OFMK_XCD_TILES_MIN_BYTES 1194393600ull      /* 192 x 1080 x 1920 x 3 */
/* DwtDctSvd read-outs (ofmk_svd_detect_rgb8, ofmk_svd_embed_detect_rgb8) only: `counts` is the PARTIAL form, device int32
 * [n][tiles][L] with tiles = ofmk_svd_count_tiles(H, W, blk) -- every workgroup of the frame kernel STORES the L sums of its own
 * tile, so the launch clears nothing first (no fill dispatch, no global atomics) and the buffer may hold anything before the
 * call.  ofmk_payloads_from_partial_counts adds the tiles up and runs DeShuffler.degenerate's epilogue
 * (de_shuffler.py:17-22; dwt_dct_svd_decoder.py:12-37 produced the bits).  L <= 2048 (else OFMK_E_ARG: use plain counts);
 * every other entry point ignores the flag. */
#define OFMK_F_PARTIAL_COUNTS 8u
/* Bytes of device scratch needed to process `frames_in_flight` frames per internal chunk.
 * Any workspace >= ofmk_workspace_bytes(1, H, W) is accepted; the engine sizes its chunks to
 * what fits.  Bigger chunks are faster (fewer launches, shorter tails): keeping a chunk resident
 * in the 256 MiB Infinity Cache between the two passes was measured NOT to pay. */
size_t ofmk_workspace_bytes(int frames_in_flight, int H, int W);

/* ---- embed: replaces Embedder.__mark_frame + DctEncoder.encode for a batch of frames ------
 * src/offmark/video/embedder.py:33-39, src/offmark/embed/dct_encoder.py:18-39.
 *   in, out   device u8 [n][H][W][3]; out may alias in (in-place)
 *   wm        device u8 [n_wm][N] of 0/1, N = H*W/64 (DctEncoder.read_wm keeps row 0 of the
 *             generator's (1,N) array; n_wm > 1 lets segments carry different payloads)
 *   wm_row    device int32 [n] giving the wm row of each frame, or NULL = row 0 for all.  The
 *             reference has one watermark per encoder (dct_encoder.py:10-11); the row map is this
 *             build's extension and so is its safety: the kernels clamp every entry into
 *             [0, n_wm) (an out-of-range entry reads the nearest valid row, never out of bounds)
 *   alpha     DctEncoder(alpha=20)
 *   chunk_frames  frames per internal chunk, 0 = as many as the workspace holds            */
int ofmk_embed_rgb8(const uint8_t *in, uint8_t *out, int n, int H, int W,
                    const uint8_t *wm, int n_wm, const int32_t *wm_row, double alpha,
                    int chunk_frames, void *workspace, size_t workspace_bytes, void *stream,
                    const ofmk_opts *opts);

/* ---- detect: replaces Extractor.__check_frame + DctDecoder.decode + the bits[i::L] sums ----
 * src/offmark/video/extractor.py:30-34, src/offmark/extract/dct_decoder.py:10-27,
 * src/offmark/degenerator/de_shuffler.py:17-18.
 *   counts    device int32 [n][L]: number of 1 bits among raw_bits[i::L] (host finishes
 *             DeShuffler.degenerate: mean, un-permute, mid-range threshold)
 *   bits      device u8 [n][N] raw per-block bits (DctDecoder.decode's array), or NULL     */
int ofmk_detect_rgb8(const uint8_t *in, int n, int H, int W, int L, double alpha,
                     int32_t *counts, uint8_t *bits,
                     int chunk_frames, void *workspace, size_t workspace_bytes, void *stream,
                     const ofmk_opts *opts);

/* ---- soft-decision read-out (BUILD EXTENSION, not reference semantics) -------------
 * soft: device int64 [n][L]; soft[f][i] = sum over blocks c with c mod L == i of round(-cos(pi*C21/step) * 2^14):
 * positive means position i reads as 1, the magnitude is a confidence.  Sums over frames of a segment can be
 * added before thresholding at 0 (offmark.dist.vote.soft_vote).  The reference's hard decision stays the
 * default everywhere. */
int ofmk_detect_soft_rgb8(const uint8_t *in, int n, int H, int W, int L, double alpha, long long *soft,
                          int chunk_frames, void *workspace, size_t workspace_bytes, void *stream,
                          const ofmk_opts *opts);

/* ---- embed then detect the produced frames, chunk by chunk (mark + verify) ---------------
 * The shape of tests/mark_video_to_hls.py:356-389 (verify every marked copy).  Same results as
 * ofmk_embed_rgb8 followed by ofmk_detect_rgb8 on `out`.  By default the mark kernel also analyzes
 * the marked block it still holds in registers, so detect's read of the frame is saved
 * (opts->flags & OFMK_F_SEPARATE_DETECT runs the literal two-call sequence instead). */
int ofmk_embed_detect_rgb8(const uint8_t *in, uint8_t *out, int n, int H, int W,
                           const uint8_t *wm, int n_wm, const int32_t *wm_row, double alpha,
                           int L, int32_t *counts, uint8_t *bits,
                           int chunk_frames, void *workspace, size_t workspace_bytes, void *stream,
                           const ofmk_opts *opts);

/* ---- DwtDctSvd codec (what tests/mark.py and tests/detect.py construct) -----------------------
 * src/offmark/embed/dwt_dct_svd_encoder.py:19-45 (Haar LL of channel 1 -> 4x4 blocks -> DCT -> SVD ->
 * s[0] = (s[0] // scale + 0.25 + 0.5*bit) * scale -> back) and
 * src/offmark/extract/dwt_dct_svd_decoder.py:12-37 (bit = (s[0] % scale) > scale/2), blk = 4.
 *   scales   HOST array of 3 doubles, one per YUV channel as in DwtDctSvdEncoder(scales=[0,15,0])
 *            (dwt_dct_svd_encoder.py:6,19-26): every channel with a positive scale is marked with the same
 *            watermark; the read-out is channel 1's (dwt_dct_svd_decoder.py:24 returns wm_bits[1]), so
 *            detection with scales[1] <= 0 yields zeros, as in the reference.  A positive scale must be a normal
 *            float32 >= 1e-3 after conversion (smaller steps are below the float32 resolution of typical top
 *            singular values; rejected with OFMK_E_ARG), NaN / infinities are rejected.
 *   blk      DwtDctSvdEncoder(blk=4): the LL block size, 4 (the reference's default: 8x8 pixel tiles, one bit per tile,
 *            N = H*W/64 bits) or 8 (16x16 pixel tiles: tile c takes wm[c], so the first quarter of the watermark row is
 *            used, dwt_dct_svd_encoder.py:29-40, and `bits` is [n][H*W/256], dwt_dct_svd_decoder.py:14).  Other values:
 *            OFMK_E_ARG (blk < 4 indexes past the reference's own watermark; larger blocks are not built).
 * Same frame/watermark/counts/bits conventions as the DCT entry points; no workspace (this codec has no
 * frame-global dependency: one pass).                                                            */
int ofmk_svd_embed_rgb8(const uint8_t *in, uint8_t *out, int n, int H, int W,
                        const uint8_t *wm, int n_wm, const int32_t *wm_row, const double *scales, int blk, void *stream,
                        const ofmk_opts *opts);
int ofmk_svd_detect_rgb8(const uint8_t *in, int n, int H, int W, int L, const double *scales, int blk,
                         int32_t *counts, uint8_t *bits, void *stream, const ofmk_opts *opts);
int ofmk_svd_embed_detect_rgb8(const uint8_t *in, uint8_t *out, int n, int H, int W,
                               const uint8_t *wm, int n_wm, const int32_t *wm_row, const double *scales, int blk,
                               int L, int32_t *counts, uint8_t *bits, void *stream, const ofmk_opts *opts);
/* ---- soft-decision read-out of the DwtDctSvd codec (BUILD EXTENSION, not reference semantics) ---------------------
 * The reference's decoder thresholds s0 mod scale at scale/2, one bit per unit (an 8x8 pixel block for blk 4, a 16x16 tile for
 * blk 8); its encoder puts a 0 at (k + 1/4) scale and a 1 at (k + 3/4) scale.  This call keeps the residue: with s0 the top
 * singular value ofmk_svd_detect_rgb8 forms, r = s0 mod scale (the float32 the hard bit compares with scale/2) and
 * u = 2 r/scale - 1,
 *     m = round(sin(pi u) * 2^14) = round(-sin(2 pi s0 / scale) * 2^14)
 * is -2^14 where a 0 was written, +2^14 where a 1 was, 0 on the thresholds; m > 0 implies ofmk_svd_detect_rgb8's bit is 1 and
 * m < 0 that it is 0, exactly.
 *   soft     device int64 [n][L]; soft[f][i] = sum of m over the units c of frame f with c mod L == i -- the convention of
 *            ofmk_detect_soft_rgb8: positive reads as 1, sums over the frames of a segment may be added before thresholding at
 *            0 (offmark.dist.vote.soft_vote).  Cleared by the call whatever it held.  scales[1] <= 0: all zeros, as the hard
 *            read-out.  blk 8 covers the tiles only: fringe pixels contribute nothing.
 * `scales`, `blk`, L >= 1 and the argument checks (OFMK_E_ARG before any HIP call) as ofmk_svd_detect_rgb8; no partial form:
 * OFMK_F_PARTIAL_COUNTS is ignored.  Launches are timed as kind 4 (svd).  The reference's hard decision stays the default
 * everywhere. */
int ofmk_svd_detect_soft_rgb8(const uint8_t *in, int n, int H, int W, int L, const double *scales, int blk,
                              long long *soft, void *stream, const ofmk_opts *opts);
/* ---- block-grid resync: reading CROPPED frames (BUILD EXTENSION, not reference semantics) ---------------------------------
 * A crop moves the phase of the 8x8 unit grid (64 possibilities) and changes the frame's block count, which scrambles the
 * position rule (unit index mod L).  DwtDctSvd has no frame-global dependency: a unit's read-out depends on its own 8x8 pixels
 * only, so at the right phase a cropped frame's units are bit for bit the marked frame's.  Two calls, both for blk 4, YUV
 * channel 1 and interleaved u8 RGB frames of any H, W >= 8 (no multiple of 8 needed):
 *
 * ofmk_svd_sync_scores_rgb8: the dense phase search.
 *   scores   device int64 [n][64]; scores[f][8*py + px] = sum of |m| over the full 8x8 windows of frame f with top-left pixel
 *            (py + 8i, px + 8j), i < (H - py) / 8, j < (W - px) / 8; m is exactly the unit metric of ofmk_svd_detect_soft_rgb8
 *            (blk 4) on that window.  A phase without a full window scores 0.  Cleared by the call whatever it held.
 *            Divided by 2^14 * windows, a marked grid scores near 1 and any other grid (or unmarked content) near 0.7; flat
 *            content carries no phase information (offmark.resync.best_phase).
 *   One frame read and one solver run per pixel origin, instead of 64 read-outs of 64 shifted copies.
 *   OFMK_E_ARG before any HIP call: null pointers, n <= 0, H or W < 8, H*W >= 2^28, blk != 4, a nan / inf scale, a positive scale
 *   below 1e-3, scales[1] <= 0, unknown flag bits.
 *
 * ofmk_svd_detect_soft_window_rgb8: the soft read-out of the units at phase (py, px), with the positions of a wider canvas.
 *   py, px        0..7; unit (i, j) is the 8x8 block at pixel (py + 8i, px + 8j), rows = (H - py) / 8, cols = (W - px) / 8 units;
 *                 read through the frame's own pitch (no copy of the window)
 *   canvas_cols   units per row of the frame the positions refer to (the uncropped frame's W / 8); >= cols
 *   base          >= 0; unit (i, j) is added into position (base + i*canvas_cols + j) mod L; base + rows*canvas_cols < 2^31
 *   soft          device int64 [n][L], cleared by the call; scales[1] <= 0: all zeros
 *   With py = px = 0, canvas_cols = W / 8, base = 0 and H, W multiples of 8 this is ofmk_svd_detect_soft_rgb8, integer for
 *   integer.  OFMK_E_ARG: the soft call's checks, a phase outside 0..7, no full unit, canvas_cols < cols, base < 0, the 2^31
 *   bound, blk != 4.
 * Both are graph capturable and timed as kind 4 (svd); OFMK_F_PARTIAL_COUNTS and the tile-order flags are ignored. */
int ofmk_svd_sync_scores_rgb8(const uint8_t *in, int n, int H, int W, const double *scales, int blk, long long *scores,
                              void *stream, const ofmk_opts *opts);
int ofmk_svd_detect_soft_window_rgb8(const uint8_t *in, int n, int H, int W, int py, int px, int canvas_cols, int base, int L,
                                     const double *scales, int blk, long long *soft, void *stream, const ofmk_opts *opts);
/* ---- block-grid resync for the DCT codec (BUILD EXTENSION, not reference semantics) -----------------------------------------
 * The same two calls for the DCT codec, on interleaved u8 RGB frames of any H, W >= 8.  This codec HAS a frame-global
 * dependency: the luminance mask's frame mean.  A decoder takes masks and mean from the frame as received, so a phase is read
 * exactly as ofmk_detect_soft_rgb8 reads the contiguous crop that holds the phase's full blocks, frame[py : py + 8*rows,
 * px : px + 8*cols], rows = (H - py) / 8, cols = (W - px) / 8 -- with the mean of THAT crop.  The right phase therefore reads
 * near, not at, +-2^14 per block (the leak's mean differs from the marked frame's; the marking itself moved the masks).
 *
 * ofmk_sync_workspace_bytes: scratch of the dense search for `frames_in_flight` frames (12 bytes per pixel origin and 64 sums
 *   per frame); 0 on bad arguments (frames_in_flight < 1, H or W < 8, H*W >= 2^28).
 *
 * ofmk_sync_scores_rgb8: the dense phase search.
 *   scores   device int64 [n][64]; scores[f][8*py + px] = sum over the blocks of that crop of |m|, m the per-block metric of
 *            ofmk_detect_soft_rgb8(crop, alpha), integer for integer.  A phase without a full window scores 0.  Cleared by the
 *            call whatever it held.  Divided by 2^14 * blocks, a marked grid scores near 0.99 and the other grids near 0.8
 *            (C21 is a low-frequency coefficient: neighbouring phases correlate); offmark.resync.best_phase.
 *   workspace / workspace_bytes / chunk_frames   as every DCT call, sized by ofmk_sync_workspace_bytes; frames go through in
 *            chunks of min(chunk_frames, what fits, 65535).  OFMK_E_WORKSPACE below ofmk_sync_workspace_bytes(1, H, W).
 *   Per chunk two launches: every pixel origin's 8x8 analysis and the 64 per-phase sums of the block DCs (timed as kind 0,
 *   analyze), then every origin's metric under its phase's mean (kind 1, finalize).  One frame read, instead of 64 read-outs of
 *   64 shifted copies.
 *   OFMK_E_ARG before any HIP call: null pointers, n <= 0, H or W < 8, H*W >= 2^28, a nan / inf / non-positive alpha, unknown
 *   flag bits, a null or misaligned workspace.
 *
 * ofmk_detect_soft_window_rgb8: the soft read-out of the blocks at phase (py, px), with the positions of a wider canvas.
 *   py, px, canvas_cols, base, soft   as ofmk_svd_detect_soft_window_rgb8; read through the frame's own pitch (no copy)
 *   workspace   of ofmk_workspace_bytes(frames_in_flight, 8*rows, 8*cols): the WINDOW's blocks
 *   With py = px = 0, canvas_cols = W / 8, base = 0 and H, W multiples of 8 this is ofmk_detect_soft_rgb8, integer for integer.
 *   Per chunk: the analyze kernel on the window (kind 0), the soft finalize with canvas positions (kind 1).
 *   OFMK_E_ARG: the checks above, L < 1, a phase outside 0..7, no full unit at the phase, canvas_cols < cols, base < 0,
 *   base + rows*canvas_cols >= 2^31.
 * Both allocate nothing, synchronise nothing and are graph capturable; the tile-order flags are ignored. */
size_t ofmk_sync_workspace_bytes(int frames_in_flight, int H, int W);
int ofmk_sync_scores_rgb8(const uint8_t *in, int n, int H, int W, double alpha, long long *scores,
                          int chunk_frames, void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts);
int ofmk_detect_soft_window_rgb8(const uint8_t *in, int n, int H, int W, int py, int px, int canvas_cols, int base, int L,
                                 double alpha, long long *soft,
                                 int chunk_frames, void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts);
/* ---- C differently marked copies of the same frames in one pass (the A/B workflow) ----------------------------------
 * tests/mark_video_to_hls.py:331-342 decodes every segment once per copy and marks it with payload segment(4b)||copy(4b).
 * These calls read the frames once, do the part of the codec that does not depend on the watermark bit once (DCT: analyze's
 * records, masks and step; DwtDctSvd: the Haar LL band and top singular triple per tile) and write every copy.
 *   out      device u8 [copies][n][H][W][3], copy-major; must not overlap `in` (no in-place: OFMK_E_ARG)
 *   copies   1..16 (a payload's copy field has 4 bits)
 *   wm_rows  device int32 [copies][n]: entry [c][f] is the watermark row of frame f in copy c, clamped into [0, n_wm) as wm_row
 *            is; NULL = copy c uses row c (clamped) for every frame
 * Exact semantics, byte for byte:
 *   ofmk_embed_copies_rgb8: copy c == ofmk_embed_rgb8(in, wm, n_wm, wm_rows + c*n, alpha), the fringe pixels of an H or W that is
 *     not a multiple of 8 included (copied from `in` into every copy).  `chunk_frames` / `workspace` as ofmk_embed_rgb8: the
 *     analysis records are shared by all copies, so ofmk_workspace_bytes(chunk, H, W) is all it needs (less than
 *     ofmk_workspace_bytes(1, H, W): OFMK_E_WORKSPACE).  Tile-order flags as ofmk_embed_rgb8 (a permutation: same bytes).
 *     Launches are timed as kind 2 (mark) and 0 (analyze).
 *   ofmk_svd_embed_copies_rgb8: copy c == ofmk_svd_embed_rgb8(in, wm, n_wm, wm_rows + c*n, scales, blk).  With `counts` or
 *     `bits` (verify; L >= 1): the counts and bits of copy c are what ofmk_svd_embed_detect_rgb8 returns for that copy (by that
 *     function's contract, ofmk_svd_detect_rgb8 of the copy): counts [copies][n][L], or with OFMK_F_PARTIAL_COUNTS
 *     [copies][n][tiles][L] (tiles = ofmk_svd_count_tiles(H, W, blk), L <= 2048, counts non-null); bits [copies][n][bits per frame]
 *     (H*W/64 for blk 4, H*W/256 for blk 8).  Both NULL: no verify, L is ignored.  blk 4 runs one fused copies kernel; blk 8
 *     runs the single-copy launches once per copy (the same results, no saving).  Launches are timed as kind 4 (svd).
 *   With copies == 1 each call equals its single-copy counterpart; no result depends on chunk_frames, the workspace size or
 *   the tile order.  Arguments are checked before any HIP call (OFMK_E_ARG): as the single-copy calls, plus the range of
 *   copies and the overlap of out with in. */
int ofmk_embed_copies_rgb8(const uint8_t *in, uint8_t *out, int copies, int n, int H, int W,
                           const uint8_t *wm, int n_wm, const int32_t *wm_rows, double alpha,
                           int chunk_frames, void *workspace, size_t workspace_bytes, void *stream,
                           const ofmk_opts *opts);
int ofmk_svd_embed_copies_rgb8(const uint8_t *in, uint8_t *out, int copies, int n, int H, int W,
                               const uint8_t *wm, int n_wm, const int32_t *wm_rows, const double *scales, int blk,
                               int L, int32_t *counts, uint8_t *bits, void *stream, const ofmk_opts *opts);
/* ---- the DCT codec's copies with the verify of every copy in the same pass -----------------------------------------------------
 * tests/mark_video_to_hls.py:356-389 verifies every marked copy.  ofmk_embed_detect_copies_rgb8 is ofmk_embed_copies_rgb8 plus the
 * read-out of every copy from the pixels the mark kernel still holds (as ofmk_embed_detect_rgb8 does for one copy): per chunk one
 * analysis of the input, one fused launch that writes every copy and every copy's block records, and the finalize of each copy's
 * records (one small launch per copy) -- 6 + 3 * copies bytes per pixel instead of 6 + 6 * copies for ofmk_embed_copies_rgb8
 * followed by ofmk_detect_rgb8 of each copy.
 *   out      device u8 [copies][n][H][W][3]: byte for byte what ofmk_embed_copies_rgb8 writes, fringe pixels included
 *   counts   device int32 [copies][n][L], bits device u8 [copies][n][N] (N = H*W/64; entries past (H/8)*(W/8) are 0); either may be
 *            NULL, not both.  For copy c they are what ofmk_embed_detect_rgb8(in, ..., wm_rows + c*n, ...) returns -- by that
 *            function's contract ofmk_detect_rgb8 of out[c] -- integer for integer.  They may hold anything before the call: the
 *            fused kernel clears the sums finalize adds into (no fill dispatch).
 *   workspace  every copy's marked frame has its own frame mean, so every copy has its own records next to the input's:
 *            ofmk_copies_workspace_bytes(frames_in_flight, copies, H, W) bytes (0 on bad arguments; monotone in frames_in_flight
 *            and in copies; >= ofmk_workspace_bytes(frames_in_flight, H, W)).  Any workspace >= ofmk_copies_workspace_bytes(1,
 *            copies, H, W) is accepted and the call sizes its chunks to what fits; a smaller one: OFMK_E_WORKSPACE.
 *   OFMK_F_SEPARATE_DETECT runs the literal sequence instead -- the non-fused copies mark, then analyze + finalize of each written
 *   copy -- with the same results.  Tile-order flags as ofmk_embed_copies_rgb8.  Launches are timed as kind 3 (the fused launch), 0
 *   (analyze) and 1 (finalize); the separate route's mark as kind 2.
 *   With copies == 1 the call equals ofmk_embed_detect_rgb8; no result depends on chunk_frames, the workspace size or the tile
 *   order.  Arguments are checked before any HIP call (OFMK_E_ARG): as ofmk_embed_copies_rgb8, plus L >= 1 and a non-NULL counts
 *   or bits as ofmk_embed_detect_rgb8.  The call only enqueues (no allocation, no synchronisation), so it captures into a hipGraph. */
size_t ofmk_copies_workspace_bytes(int frames_in_flight, int copies, int H, int W);
int ofmk_embed_detect_copies_rgb8(const uint8_t *in, uint8_t *out, int copies, int n, int H, int W,
                                  const uint8_t *wm, int n_wm, const int32_t *wm_rows, double alpha,
                                  int L, int32_t *counts, uint8_t *bits,
                                  int chunk_frames, void *workspace, size_t workspace_bytes, void *stream,
                                  const ofmk_opts *opts);
/* plugin level, float32 YUV [n][H][W][3] (n <= 65535): encode mutates the marked channels; decode fills bits */
int ofmk_svd_encode_yuv32f(float *yuv, int n, int H, int W,
                           const uint8_t *wm, int n_wm, const int32_t *wm_row, const double *scales, int blk, void *stream,
                           const ofmk_opts *opts);
int ofmk_svd_decode_yuv32f(const float *yuv, int n, int H, int W, const double *scales, int blk, uint8_t *bits, void *stream,
                           const ofmk_opts *opts);

/* ---- planar 8-bit YUV 4:2:0 on either side of the DCT codec ------------------------------
 * The reference moves rgb24 over pipes and has ffmpeg convert to yuv420p on the way out
 * (src/offmark/video/frame_reader.py:42-64, src/offmark/video/frame_writer.py:33-34).  These entry points take and
 * produce the 4:2:0 planes themselves, so a decoder's output stays on the device and HBM / PCIe carry 1.5 instead
 * of 3 bytes per pixel each way.  The result is, bit for bit,
 *     ofmk_yuv420_to_rgb8 -> ofmk_embed_rgb8 / ofmk_detect_rgb8 -> ofmk_rgb8_to_yuv420
 * with the conversions fused into the kernels' loads and stores.  The conversion is BUILD-DEFINED (swscale is not
 * available here and its rounding is not claimed): BT.601 studio swing in float32 fused multiply-adds, clip to
 * [0,255], round half to even; chroma is replicated over its 2x2 pixels on the way in and is the conversion of the
 * 2x2 mean RGB on the way out (csrc/planar_kernels.hiph, restated in oracle/offmark_oracle.py).
 *   layout  OFMK_YUV_I420: per frame [Y: H*W][U: H/2*W/2][V: H/2*W/2];  OFMK_YUV_NV12: [Y: H*W][UV interleaved: H/2*W]
 *           frames are consecutive, 1.5*H*W bytes each; H and W must be multiples of 8, buffers 8-byte aligned
 *   ofmk_embed_detect_yuv420's counts/bits are those of a reader of the WRITTEN planes (== ofmk_detect_yuv420(out)). */
#define OFMK_YUV_I420 0
#define OFMK_YUV_NV12 1
int ofmk_embed_yuv420(const uint8_t *in, uint8_t *out, int layout, int n, int H, int W,
                      const uint8_t *wm, int n_wm, const int32_t *wm_row, double alpha,
                      int chunk_frames, void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts);
int ofmk_detect_yuv420(const uint8_t *in, int layout, int n, int H, int W, int L, double alpha,
                       int32_t *counts, uint8_t *bits,
                       int chunk_frames, void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts);
int ofmk_embed_detect_yuv420(const uint8_t *in, uint8_t *out, int layout, int n, int H, int W,
                             const uint8_t *wm, int n_wm, const int32_t *wm_row, double alpha,
                             int L, int32_t *counts, uint8_t *bits,
                             int chunk_frames, void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts);
/* The DCT codec's soft-decision read-out (BUILD EXTENSION, see ofmk_detect_soft_rgb8) on the same planes: integer for integer,
 *     ofmk_detect_soft_yuv420 == ofmk_detect_soft_rgb8(ofmk_yuv420_to_rgb8(in)).
 * Arguments as ofmk_detect_soft_rgb8 plus `layout`; checked as ofmk_detect_yuv420 checks them. */
int ofmk_detect_soft_yuv420(const uint8_t *in, int layout, int n, int H, int W, int L, double alpha, long long *soft,
                            int chunk_frames, void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts);
/* The DwtDctSvd codec on the same 4:2:0 planes.  `scales`, `blk`, `wm` / `n_wm` / `wm_row`, `L` / `counts` / `bits` and `opts`
 * (OFMK_F_PARTIAL_COUNTS included: tiles = ofmk_svd_count_tiles(H, W, blk)) as ofmk_svd_*_rgb8; `layout` and the planes as
 * ofmk_*_yuv420 above; no workspace.  The result is, bit for bit,
 *     ofmk_svd_embed_yuv420         == ofmk_rgb8_to_yuv420(ofmk_svd_embed_rgb8(ofmk_yuv420_to_rgb8(in)))
 *     ofmk_svd_detect_yuv420        == ofmk_svd_detect_rgb8(ofmk_yuv420_to_rgb8(in))
 *     ofmk_svd_embed_detect_yuv420  == `out` as the embed; counts / bits == ofmk_svd_detect_yuv420(out), what a reader of the
 *                                      WRITTEN planes sees (the verify reads out with the stand-alone read-out's tolerance)
 * in one tile-local pass: 1.5 B/px read and 1.5 B/px written instead of the chain's 15 B/px (embed) and 7.5 B/px (detect).
 *   blk = 8  the tiles cover only the first 16*floor(H/16) rows and 16*floor(W/16) columns; the pixels outside come out as the
 *            chain leaves them: the planes -> RGB -> planes round trip of the input (not the input bytes), also when in == out
 *            (one more launch, timed as "svd" like the tile launch).  `bits` is [n][H*W/256]; entries past the tiles are 0.
 *   blk = 4  `bits` is [n][H*W/64]; with H and W multiples of 8 there is no fringe.
 *   in == out is allowed.  Arguments are checked before any HIP call (OFMK_E_ARG): as the rgb8 SVD calls, plus the layout, H and W
 *   multiples of 8 and 8-byte aligned frame buffers. */
int ofmk_svd_embed_yuv420(const uint8_t *in, uint8_t *out, int layout, int n, int H, int W,
                          const uint8_t *wm, int n_wm, const int32_t *wm_row, const double *scales, int blk,
                          void *stream, const ofmk_opts *opts);
int ofmk_svd_detect_yuv420(const uint8_t *in, int layout, int n, int H, int W, int L, const double *scales, int blk,
                           int32_t *counts, uint8_t *bits, void *stream, const ofmk_opts *opts);
int ofmk_svd_embed_detect_yuv420(const uint8_t *in, uint8_t *out, int layout, int n, int H, int W,
                                 const uint8_t *wm, int n_wm, const int32_t *wm_row, const double *scales, int blk,
                                 int L, int32_t *counts, uint8_t *bits, void *stream, const ofmk_opts *opts);
/* The DwtDctSvd soft-decision read-out (BUILD EXTENSION, see ofmk_svd_detect_soft_rgb8) on 4:2:0 planes: the same loads and LL
 * band as ofmk_svd_detect_yuv420, so, integer for integer,
 *     ofmk_svd_detect_soft_yuv420 == ofmk_svd_detect_soft_rgb8(ofmk_yuv420_to_rgb8(in)).
 * blk 8 covers the tiles only: fringe pixels contribute nothing.  Arguments are checked as ofmk_svd_detect_yuv420 checks them
 * (`soft` in place of counts / bits); OFMK_F_PARTIAL_COUNTS is ignored. */
int ofmk_svd_detect_soft_yuv420(const uint8_t *in, int layout, int n, int H, int W, int L, const double *scales, int blk,
                                long long *soft, void *stream, const ofmk_opts *opts);
/* ---- C differently marked copies of the same 4:2:0 frames in one pass: the copies calls above on planes -----------------------
 * The workflow the copies calls serve (tests/mark_video_to_hls.py:331-342) gets its frames from a decoder and hands them to an
 * encoder, so they arrive and leave as 4:2:0 planes.  These calls read the planes once, do what does not depend on the watermark
 * bit once (DCT: analyze's records, and every pixel's planes -> RGB -> Y / U / V conversion; DwtDctSvd: the LL band and top singular
 * triple per tile) and write every copy: 1.5 + 1.5 * copies bytes per pixel (csrc/planar_copies_kernels.hiph).
 *   in       device u8 [n] frames of 1.5*H*W bytes, `layout` as ofmk_*_yuv420
 *   out      device u8 [copies][n][1.5*H*W], copy-major, the same layout as `in`; must not overlap `in` (OFMK_E_ARG)
 *   copies   1..16;  wm_rows  device int32 [copies][n], clamped into [0, n_wm); NULL = copy c uses row c (clamped) for every frame
 * Exact semantics, byte for byte:
 *   ofmk_embed_copies_yuv420: copy c == ofmk_embed_yuv420(in, layout, wm, n_wm, wm_rows + c*n, alpha).  `chunk_frames` / `workspace`
 *     as ofmk_embed_yuv420: the records are shared by all copies, ofmk_workspace_bytes(chunk, H, W) is all it needs (less than
 *     ofmk_workspace_bytes(1, H, W): OFMK_E_WORKSPACE).  Launches are timed as kind 5 (planar analyze, once per chunk) and
 *     6 (planar mark, every copy of the chunk in one launch).
 *   ofmk_svd_embed_copies_yuv420: copy c == ofmk_svd_embed_yuv420(in, layout, wm, n_wm, wm_rows + c*n, scales, blk), with blk 8 the
 *     fringe's 4:2:0 round trip included in every copy.  With `counts` or `bits` (verify; L >= 1): the counts and bits of copy c are
 *     what ofmk_svd_embed_detect_yuv420 returns for that copy (by that function's contract, ofmk_svd_detect_yuv420 of the copy):
 *     counts [copies][n][L], or with OFMK_F_PARTIAL_COUNTS [copies][n][tiles][L] (tiles = ofmk_svd_count_tiles(H, W, blk),
 *     L <= 2048, counts non-null); bits [copies][n][bits per frame] (H*W/64 for blk 4, H*W/256 for blk 8).  Both NULL: no verify,
 *     L is ignored.  blk 4 runs one fused copies kernel; blk 8 runs the single-copy launches once per copy (the same results, no
 *     saving).  Launches are timed as kind 4 (svd).
 *   With copies == 1 each call equals its single-copy counterpart; no result depends on chunk_frames or the workspace size.
 *   Arguments are checked before any HIP call (OFMK_E_ARG): as the single-copy planar calls (layout, H and W multiples of 8,
 *   8-byte aligned buffers, scales, blk, L, partial counts), plus the range of copies and the overlap of out with in. */
int ofmk_embed_copies_yuv420(const uint8_t *in, uint8_t *out, int layout, int copies, int n, int H, int W,
                             const uint8_t *wm, int n_wm, const int32_t *wm_rows, double alpha,
                             int chunk_frames, void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts);
int ofmk_svd_embed_copies_yuv420(const uint8_t *in, uint8_t *out, int layout, int copies, int n, int H, int W,
                                 const uint8_t *wm, int n_wm, const int32_t *wm_rows, const double *scales, int blk,
                                 int L, int32_t *counts, uint8_t *bits, void *stream, const ofmk_opts *opts);
/* ---- the copies calls with the SOFT read-out of every copy in the same pass (BUILD EXTENSION, not reference semantics) --------
 * Each call is its counterpart above -- ofmk_embed_detect_copies_rgb8, ofmk_svd_embed_copies_rgb8, ofmk_svd_embed_copies_yuv420 --
 * with one more output after `bits`:
 *   soft     device int64 [copies][n][L], required; L >= 1.  soft[c] is the stand-alone soft read-out of the written copy, integer
 *            for integer: ofmk_detect_soft_rgb8(out[c], alpha), ofmk_svd_detect_soft_rgb8(out[c], scales, blk) and
 *            ofmk_svd_detect_soft_yuv420(out[c], layout, scales, blk) respectively -- taken from the pixels (DwtDctSvd blk 4: the
 *            verify's LL block and the stand-alone read-out's tight s0) or the block records (DCT codec) the copies kernels still hold,
 *            so no written copy is read back.  Cleared by the call whatever it held.  scales[1] <= 0: all zeros.  No partial form.
 *   out, counts, bits   exactly what the counterpart writes, byte for byte and integer for integer (OFMK_F_PARTIAL_COUNTS applies
 *            to `counts` of the DwtDctSvd calls); counts and bits may BOTH be NULL here: the soft sums alone.
 *   DCT codec: per chunk and copy the soft finalize of the copy's records next to the hard one (two small launches per copy,
 *   kind 1); workspace of ofmk_copies_workspace_bytes; OFMK_F_SEPARATE_DETECT runs the literal sequence, ofmk_detect_soft_rgb8 of
 *   each written copy included, with the same results.  DwtDctSvd blk 4: one fused launch for all copies, hard and soft sums
 *   through an LDS histogram each (L > 2048: global atomics); blk 8: the single-copy launches and the stand-alone soft read-out
 *   once per copy (the same results, no saving).  Launches are timed under the kinds of the counterparts.
 *   With copies == 1 the results equal the single-copy embed (+ verify) plus the soft read-out of its output; nothing depends on
 *   chunk_frames, the workspace size, the tile order or OFMK_F_SEPARATE_DETECT.  Arguments are checked before any HIP call
 *   (OFMK_E_ARG): the counterpart's checks plus a non-NULL `soft` and L >= 1.  The calls only enqueue (no allocation, no
 *   synchronisation), so they capture into a hipGraph. */
int ofmk_embed_detect_copies_soft_rgb8(const uint8_t *in, uint8_t *out, int copies, int n, int H, int W,
                                       const uint8_t *wm, int n_wm, const int32_t *wm_rows, double alpha,
                                       int L, int32_t *counts, uint8_t *bits, long long *soft,
                                       int chunk_frames, void *workspace, size_t workspace_bytes, void *stream,
                                       const ofmk_opts *opts);
int ofmk_svd_embed_copies_soft_rgb8(const uint8_t *in, uint8_t *out, int copies, int n, int H, int W,
                                    const uint8_t *wm, int n_wm, const int32_t *wm_rows, const double *scales, int blk,
                                    int L, int32_t *counts, uint8_t *bits, long long *soft, void *stream, const ofmk_opts *opts);
int ofmk_svd_embed_copies_soft_yuv420(const uint8_t *in, uint8_t *out, int layout, int copies, int n, int H, int W,
                                      const uint8_t *wm, int n_wm, const int32_t *wm_rows, const double *scales, int blk,
                                      int L, int32_t *counts, uint8_t *bits, long long *soft, void *stream, const ofmk_opts *opts);
/* ---- the DCT codec's copies on 4:2:0 planes with the verify of every copy in the same pass, hard and soft ----------------------
 * ofmk_embed_detect_copies_yuv420 is ofmk_embed_copies_yuv420 plus the read-out of every copy from the pixels the mark kernel
 * still holds, as ofmk_embed_detect_yuv420 does for one copy and ofmk_embed_detect_copies_rgb8 for RGB frames; the _soft_ call
 * adds the soft read-out (BUILD EXTENSION, see ofmk_detect_soft_rgb8) of every copy from the same records.  Per chunk: one planar
 * analysis of the input, ONE launch that writes every copy and every copy's block records, and the finalize of each copy's records
 * (small launches per copy).  A block has only two marked forms whatever `copies` is (watermark bit 0 or 1), so the launch runs
 * the fused mark + verify body once for the form of copy 0 and once more for the other form where some copy of the block takes it,
 * and stores each form into every copy that takes it (csrc/planar_copies_kernels.hiph).  No written copy is read back:
 * 3 + 1.5 * copies bytes per pixel instead of 3 + 3 * copies for ofmk_embed_copies_yuv420 followed by ofmk_detect_yuv420 of each
 * copy (3 + 4.5 * copies with ofmk_detect_soft_yuv420 of each copy as well).
 *   in, layout, copies, wm, n_wm, wm_rows, alpha   as ofmk_embed_copies_yuv420
 *   out      device u8 [copies][n][1.5*H*W]: byte for byte what ofmk_embed_copies_yuv420 writes; must not overlap `in`
 *   counts   device int32 [copies][n][L], bits device u8 [copies][n][H*W/64].  For copy c they are what
 *            ofmk_embed_detect_yuv420(in, ..., wm_rows + c*n, ...) returns -- by that function's contract ofmk_detect_yuv420 of
 *            out[c] -- integer for integer.  They may hold anything before the call: the fused kernel clears the sums finalize adds
 *            into (no fill dispatch).  ofmk_embed_detect_copies_yuv420: either may be NULL, not both.
 *            ofmk_embed_detect_copies_soft_yuv420: both may be NULL (the soft sums alone).
 *   soft     (the _soft_ call) device int64 [copies][n][L], required: soft[c] == ofmk_detect_soft_yuv420(out[c], layout, alpha),
 *            integer for integer.  Cleared by the call whatever it held.
 *   workspace  ofmk_copies_workspace_bytes(frames_in_flight, copies, H, W), as ofmk_embed_detect_copies_rgb8 (every copy keeps its
 *            own records).  Any workspace >= ofmk_copies_workspace_bytes(1, copies, H, W) is accepted and the call sizes its chunks
 *            to what fits; a smaller one -- ofmk_workspace_bytes(1, H, W) for instance -- is OFMK_E_WORKSPACE.
 *   OFMK_F_SEPARATE_DETECT runs the literal sequence instead -- the non-fused planar copies mark, then planar analyze + finalize
 *   (hard, and soft for the _soft_ call) of each written copy -- with the same results.  Launches are timed as kind 5 (planar
 *   analyze: of the input once per chunk; the separate route's of each copy), 6 (the fused launch, once per chunk; the separate
 *   route's mark) and 1 (finalize: per copy and chunk, twice where hard and soft outputs are both asked for).
 *   With copies == 1 the call equals ofmk_embed_detect_yuv420 (plus ofmk_detect_soft_yuv420 of its output); no result depends on
 *   chunk_frames, the workspace size or OFMK_F_SEPARATE_DETECT.  Arguments are checked before any HIP call (OFMK_E_ARG): as
 *   ofmk_embed_copies_yuv420 (layout, H and W multiples of 8, 8-byte aligned buffers, copies in 1..16, out not overlapping in), plus
 *   L >= 1, the non-NULL outputs above and the opts.  The calls only enqueue (no allocation, no synchronisation), so they capture
 *   into a hipGraph. */
int ofmk_embed_detect_copies_yuv420(const uint8_t *in, uint8_t *out, int layout, int copies, int n, int H, int W,
                                    const uint8_t *wm, int n_wm, const int32_t *wm_rows, double alpha,
                                    int L, int32_t *counts, uint8_t *bits,
                                    int chunk_frames, void *workspace, size_t workspace_bytes, void *stream,
                                    const ofmk_opts *opts);
int ofmk_embed_detect_copies_soft_yuv420(const uint8_t *in, uint8_t *out, int layout, int copies, int n, int H, int W,
                                         const uint8_t *wm, int n_wm, const int32_t *wm_rows, double alpha,
                                         int L, int32_t *counts, uint8_t *bits, long long *soft,
                                         int chunk_frames, void *workspace, size_t workspace_bytes, void *stream,
                                         const ofmk_opts *opts);
int ofmk_yuv420_to_rgb8(const uint8_t *yuv, uint8_t *rgb, int layout, int n, int H, int W, void *stream,
                        const ofmk_opts *opts);
int ofmk_rgb8_to_yuv420(const uint8_t *rgb, uint8_t *yuv, int layout, int n, int H, int W, void *stream,
                        const ofmk_opts *opts);
/* ---- block-grid resync on 4:2:0 planes: reading CROPPED planar frames (BUILD EXTENSION, not reference semantics) ---------------
 * The four resync calls above for frames given as planes (layout and frame size as the yuv420 calls: 1.5*H*W bytes per frame,
 * frames consecutive), both codecs, blk 4, YUV channel 1.  New here: H and W need only be EVEN and >= 8, not multiples of 8,
 * and nothing is asked of any address (W = 84 has 42-byte I420 chroma rows; 10x14 frames lie 210 bytes apart).
 *
 * Only the 16 phases with EVEN py and px exist on planes:
 *   1. a crop at even pixel offsets cuts sub-planes out of the marked planes, and the build-defined conversion replicates chroma
 *      over its 2x2 cell, so yuv420_to_rgb(crop of planes) == crop of yuv420_to_rgb(planes), byte for byte: such leaks read
 *      correctly with both codecs;
 *   2. a crop at an odd offset cannot be made on 4:2:0 planes without resampling chroma by half a sample.  Done through RGB
 *      (convert, crop at (11, 21), convert back) it destroys both codecs' marks, which live in U: measured with the oracle,
 *      phase contrast 1.017 (DwtDctSvd) and 1.005 (DCT) against 1.30 and 1.11 at the even offsets.  A property of a chroma
 *      mark under 4:2:0, not of the search.
 * So the searches run one solver / one block analysis per even pixel origin, a quarter of the RGB searches', on 1.5 B/px read
 * once and without an RGB intermediate, and every score entry with an odd py or px is 0.
 *
 * sub(py, px) below is the frame's sub-planes for the pixel window [py : py + 8*r, px : px + 8*c], r = (H - py) / 8,
 * c = (W - px) / 8: a planar frame of 8r x 8c pixels, which the existing planar calls can read.
 *
 * ofmk_svd_sync_scores_yuv420: the dense phase search of the DwtDctSvd codec.
 *   scores   device int64 [n][64], cleared by the call whatever it held.  For even py, even px, r >= 1 and c >= 1:
 *            scores[f][8*py + px] = sum of |m| over the units of sub(py, px), m exactly the unit metric of
 *            ofmk_svd_detect_soft_yuv420 (blk 4) on that sub-frame -- which is also entry 8*py + px of
 *            ofmk_svd_sync_scores_rgb8 on the converted frame (fact 1).  Every other entry (odd phases, phases without a unit)
 *            is 0 (fact 2).
 *   OFMK_E_ARG before any HIP call: the checks of ofmk_svd_sync_scores_rgb8, an unknown layout, odd H or W.
 *
 * ofmk_svd_detect_soft_window_yuv420: the soft read-out of the units of sub(py, px), with the positions of a wider canvas.
 *   py, px   0, 2, 4 or 6; unit (i, j) of sub(py, px) is added into position (base + i*canvas_cols + j) mod L; canvas_cols,
 *            base, soft and the scales as ofmk_svd_detect_soft_window_rgb8; read through the frame's own pitch (no copy)
 *   With py = px = 0, canvas_cols = W / 8, base = 0 and H, W multiples of 8 this is ofmk_svd_detect_soft_yuv420 (blk 4),
 *   integer for integer.  OFMK_E_ARG: the checks of ofmk_svd_detect_soft_window_rgb8, an unknown layout, odd H or W, odd py or px.
 * Both are timed as kind 4 (svd).
 *
 * ofmk_sync_workspace_bytes_yuv420: scratch of the DCT codec's planar search for `frames_in_flight` frames (12 bytes per even
 *   pixel origin and 16 sums per frame: at most ofmk_sync_workspace_bytes of the same shape, about a quarter of it); 0 on bad
 *   arguments (frames_in_flight < 1, H or W < 8 or odd, H*W >= 2^28).
 *
 * ofmk_sync_scores_yuv420: the dense phase search of the DCT codec.
 *   scores   as above with m the per-block metric of ofmk_detect_soft_yuv420(sub(py, px), alpha): masks and the luminance
 *            mask's frame mean come from that sub-frame, as ofmk_sync_scores_rgb8 takes them from each phase's crop.
 *   workspace / workspace_bytes / chunk_frames   as ofmk_sync_scores_rgb8, sized by ofmk_sync_workspace_bytes_yuv420;
 *            OFMK_E_WORKSPACE below ofmk_sync_workspace_bytes_yuv420(1, H, W).
 *   Per chunk two launches: every even origin's 8x8 analysis and the 16 per-phase sums of the block DCs (timed as kind 5, planar
 *   analyze), then every origin's metric under its phase's mean (kind 1, finalize).
 *   OFMK_E_ARG before any HIP call: the checks of ofmk_sync_scores_rgb8, an unknown layout, odd H or W.
 *
 * ofmk_detect_soft_window_yuv420: the soft read-out of the blocks of sub(py, px), with the positions of a wider canvas.
 *   py, px, canvas_cols, base, soft   as ofmk_svd_detect_soft_window_yuv420
 *   workspace   of ofmk_workspace_bytes(frames_in_flight, 8*r, 8*c): the WINDOW's blocks
 *   With py = px = 0, canvas_cols = W / 8, base = 0 and H, W multiples of 8 this is ofmk_detect_soft_yuv420, integer for integer.
 *   Per chunk: the planar analyze on the window (kind 5), the soft finalize with canvas positions (kind 1).
 *   OFMK_E_ARG: the checks of ofmk_detect_soft_window_rgb8, an unknown layout, odd H or W, odd py or px.
 * All four allocate nothing, synchronise nothing, are graph capturable and launch at most 65535 frames at a time; the tile-order
 * flags and OFMK_F_PARTIAL_COUNTS are ignored. */
int ofmk_svd_sync_scores_yuv420(const uint8_t *in, int layout, int n, int H, int W, const double *scales, int blk,
                                long long *scores, void *stream, const ofmk_opts *opts);
int ofmk_svd_detect_soft_window_yuv420(const uint8_t *in, int layout, int n, int H, int W, int py, int px, int canvas_cols,
                                       int base, int L, const double *scales, int blk, long long *soft, void *stream,
                                       const ofmk_opts *opts);
size_t ofmk_sync_workspace_bytes_yuv420(int frames_in_flight, int H, int W);
int ofmk_sync_scores_yuv420(const uint8_t *in, int layout, int n, int H, int W, double alpha, long long *scores,
                            int chunk_frames, void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts);
int ofmk_detect_soft_window_yuv420(const uint8_t *in, int layout, int n, int H, int W, int py, int px, int canvas_cols,
                                   int base, int L, double alpha, long long *soft,
                                   int chunk_frames, void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts);

/* ---- reading RESCALED leaks: fixed-point warp, fused geometry search, fused read-out (BUILD EXTENSION) ------------------------
 * A leak that was cropped and scaled has lost the 8x8 grid.  It is resampled back onto the marked frame's pixel grid (the CANVAS,
 * H x W) with the inverse of the crop and scale, and the canvas units are read with the unit metric of ofmk_svd_detect_soft_rgb8;
 * read in canvas coordinates, a unit has the uncropped frame's position, so no rotation is left to resolve.  Interleaved u8 RGB,
 * blk 4, YUV channel 1.  The warp is defined in integers, so every implementation agrees byte for byte:
 *
 *   ofmk_warp {ay, by, ax, bx}, Q16.  Canvas row y reads the leak (h x w) at pos = ay*y + by (int64): y0 = pos >> 16 (floor),
 *   fy = (pos >> 8) & 255; columns alike with ax, bx.  A pixel is INSIDE iff 0 <= y0 <= h-1 and 0 <= x0 <= w-1; the second taps
 *   are min(y0+1, h-1), min(x0+1, w-1).  Per channel
 *       v = ((256-fy)*((256-fx)*p00 + fx*p01) + fy*((256-fx)*p10 + fx*p11) + 32768) >> 16
 *   and 0 outside.  a = 65536, b = 0 returns the frame; b = k << 16 the frame shifted by k pixels.
 *   Required: 2^12 <= ay, ax <= 2^20 and |by|, |bx| <= 2^48 (pos then stays far inside int64), else OFMK_E_ARG.
 *   A leak of h x w made from canvas rows top:top+ch (and columns alike) has ay = round(h/ch * 65536),
 *   by = round(((0.5 - top) * h/ch - 0.5) * 65536): offmark.resync.warp_of_crop.
 *   Canvas unit (i, j), i < H/8, j < W/8, COUNTS iff all 64 of its pixels are inside; the maps are monotone, so the counting units
 *   form a rectangle [i0, i1) x [j0, j1).
 *
 * ofmk_warp_units: host only, no GPU call.  out = {i0, i1, j0, j1}, all 0 when no unit counts.  h, w, H, W >= 1 (a leak smaller
 *   than a unit may still fill units when it is upscaled), h*w and H*W < 2^28.
 * ofmk_warp_rgb8: out, device u8 [n][Hout][Wout][3], is the canvas rectangle whose top-left canvas pixel is (oy, ox); every byte
 *   is written.  geom is HOST memory.  One launch per 65535 frames, not timed.  OFMK_E_ARG: null pointers, n <= 0, h or w < 1,
 *   Hout or Wout < 1, a product >= 2^28, oy or ox outside [0, 2^28), the map's range.
 * ofmk_svd_warp_scores_rgb8: the geometry search over a given candidate list.
 *   cands    DEVICE memory, ofmk_warp [K] (an int64 [K][4] array)
 *   scores   device int64 [n][K]; scores[f][k] = sum of |m| over the counting units of frame f warped by candidate k, m exactly
 *            the unit metric ofmk_svd_detect_soft_rgb8 gives on the warped unit.  Cleared by the call whatever it held.  A
 *            candidate without a counting unit scores 0, and so does one whose map is out of range (the list is not read on the
 *            host).  Divided by 2^14 * counting units, the true geometry of a marked leak scores about 0.8 and a geometry with
 *            one crop edge off by a pixel falls to the unmarked level (offmark.resync.best_geometry).
 *   One thread per canvas unit and candidate forms the unit's 64 warped pixels in registers: no warped frame is written, one
 *   launch for up to 65535 candidates x 65535 frames (candidates in gridDim.y, frames in gridDim.z, both chunked).
 *   OFMK_E_ARG before any HIP call: null pointers, n <= 0, K < 1, h or w < 1, H or W < 8, a product >= 2^28, blk != 4, a nan / inf
 *   scale, a positive scale below 1e-3, scales[1] <= 0, unknown flag bits.
 * ofmk_svd_detect_soft_warp_rgb8: the soft read-out at one geometry (HOST memory).
 *   soft     device int64 [n][L], cleared by the call; counting unit (i, j) adds m into position (i * (W/8) + j) mod L.
 *            scales[1] <= 0 or no counting unit: all zeros.
 *   Equal, integer for integer, to ofmk_warp_rgb8 of the counting rectangle (origin (8*i0, 8*j0)) followed by
 *   ofmk_svd_detect_soft_window_rgb8 at phase (0, 0) with canvas_cols = W/8 and base = i0 * (W/8) + j0; at the identity on a frame
 *   with H, W multiples of 8 it is ofmk_svd_detect_soft_rgb8.  OFMK_E_ARG: as above, L < 1, the map's range.
 * The three device calls allocate nothing, synchronise nothing and are graph capturable; the fused ones are timed as kind 4
 * (svd); OFMK_F_PARTIAL_COUNTS and the tile-order flags are ignored. */
typedef struct ofmk_warp { int64_t ay, by, ax, bx; } ofmk_warp;
int ofmk_warp_units(int h, int w, int H, int W, const ofmk_warp *geom, int out[4]);
int ofmk_warp_rgb8(const uint8_t *in, int n, int h, int w, uint8_t *out, int Hout, int Wout, int oy, int ox,
                   const ofmk_warp *geom, void *stream, const ofmk_opts *opts);
int ofmk_svd_warp_scores_rgb8(const uint8_t *in, int n, int h, int w, int H, int W, const ofmk_warp *cands, int K,
                              const double *scales, int blk, long long *scores, void *stream, const ofmk_opts *opts);
int ofmk_svd_detect_soft_warp_rgb8(const uint8_t *in, int n, int h, int w, int H, int W, const ofmk_warp *geom, int L,
                                   const double *scales, int blk, long long *soft, void *stream, const ofmk_opts *opts);

/* ---- reading ROTATED leaks: the same warp under a 2x3 affine map (BUILD EXTENSION) ---------------------------------------------
 * The rescaled-leak calls above with a full affine map: rotation, shear, anisotropic scale, flips and 90 degree turns.  Interleaved
 * u8 RGB, blk 4, YUV channel 1.
 *
 *   ofmk_affine {ayy, ayx, by, axy, axx, bx}, Q16.  Canvas pixel (y, x) reads the leak (h x w) at
 *       pos_y = ayy*y + ayx*x + by      pos_x = axy*y + axx*x + bx      (int64)
 *   and everything else is ofmk_warp's rule, word for word: y0 = pos_y >> 16, fy = (pos_y >> 8) & 255, columns alike; INSIDE iff
 *   0 <= y0 <= h-1 and 0 <= x0 <= w-1; second taps min(y0+1, h-1), min(x0+1, w-1); per channel
 *       v = ((256-fy)*((256-fx)*p00 + fx*p01) + fy*((256-fx)*p10 + fx*p11) + 32768) >> 16
 *   and 0 outside.  ayx = axy = 0 is ofmk_warp {ayy, by, axx, bx} byte for byte.  Negative coefficients are allowed:
 *   {65536, 0, 0, 0, -65536, (w-1) << 16} returns the frame mirrored left to right.
 *   Required, else OFMK_E_ARG: the four coefficients in [-2^20, 2^20], |by|, |bx| <= 2^48 (pos then stays far inside int64) and
 *   |ayy*axx - ayx*axy| >= 2^24 (the square of ofmk_warp's smallest scale).
 *   offmark.resync.affine_of_rotation gives the map of a leak rotated and scaled about its centre.
 *   Canvas unit (i, j), i < H/8, j < W/8, COUNTS iff all 64 of its pixels are inside.  Positions are affine and the inside set is an
 *   intersection of half-planes, so that is: iff its 4 corner pixels (8i, 8j), (8i, 8j+7), (8i+7, 8j), (8i+7, 8j+7) are inside.  The
 *   counting units are convex, not a rectangle.
 *
 * ofmk_affine_units: host only, no GPU call.  out = {i0, i1, j0, j1, count}: the bounding rectangle [i0, i1) x [j0, j1) of the
 *   counting units and how many count; all 0 when none does.  Argument rules as ofmk_warp_units.
 * ofmk_warp_affine_rgb8: as ofmk_warp_rgb8 -- out is the canvas rectangle with top-left canvas pixel (oy, ox), every byte is
 *   written, geom is HOST memory, same argument rules.
 * ofmk_svd_affine_scores_rgb8: as ofmk_svd_warp_scores_rgb8 with cands DEVICE memory, ofmk_affine [K] (an int64 [K][6] array).
 *   scores is cleared by the call; a candidate out of range scores 0 (the list is not read on the host), and so does one without
 *   a counting unit.  Candidates in gridDim.y and frames in gridDim.z, chunked at 65535 and below 2^30 workgroups per launch.
 *   One thread per canvas unit and candidate, a workgroup per tile of 16 x 16 units; a pixel's two taps of one leak row are
 *   fetched together (6 adjacent bytes).  No warped frame is written.
 * ofmk_svd_detect_soft_affine_rgb8: as ofmk_svd_detect_soft_warp_rgb8 -- counting unit (i, j) adds m into position
 *   (i * (W/8) + j) mod L; soft is cleared by the call; scales[1] <= 0 or no counting unit: all zeros.  Equal, integer for integer,
 *   to ofmk_warp_affine_rgb8 of the canvas followed by the soft read-out of the counting units at their canvas positions.
 * ofmk_svd_affine_phase_scores_rgb8: the DENSE SHIFT SEARCH, for a leak that was rotated or rescaled and then cropped off-centre, so
 *   that its translation is unknown.  A shift of the canvas by whole pixels (py, px) is an exact integer change of a map's offsets,
 *       g (+) (py, px):   by' = by + ayy*py + ayx*px    bx' = bx + axy*py + axx*px
 *   and the call scores all 64 shifts by 0..7 px of every candidate: scores[f][k][8*py + px] (device int64 [n][K][64]) is the score
 *   ofmk_svd_affine_scores_rgb8 gives frame f under cands[k] (+) (py, px) on the same canvas H x W, integer for integer: the sum of
 *   |m| over units (i, j), i < H/8, j < W/8, whose canvas pixels are (py + 8i + r, px + 8j + c); a unit counts iff its four corner
 *   pixels are inside the leak.  Canvas coordinates are an index space: a shifted unit may reach past row H or column W.
 *   units[k][8*py + px] (device int64 [K][64], may be NULL) is the count ofmk_affine_units(h, w, H, W, cands[k] (+) (py, px)) returns,
 *   written once per call.  Both outputs are cleared by the call.  A candidate is in range iff all 64 shifted maps pass ofmk_affine's
 *   rules (the linear part is shared: a condition on by, bx); one that is not scores 0 in all 64 entries and has 0 units (the list is
 *   device memory and is not read on the host).  Shifts by whole units need no entry: they rotate the payload positions by a
 *   constant, which offmark.resync.align_segments resolves; sub-pixel shifts do (offmark.resync.subpixel_shifts).
 *   A workgroup owns 32 x 32 canvas pixel origins of one candidate and one frame: it warps the 39 x 39 pixels they cover once, stages
 *   their dense LL plane in LDS as ofmk_svd_sync_scores_rgb8 does and runs one solver per origin that counts, so a candidate's
 *   pixels are warped once instead of once per shift.  Arguments, chunking and flags as ofmk_svd_affine_scores_rgb8.
 * The four device calls allocate nothing, synchronise nothing and are graph capturable; all four are timed as kind 4 (svd);
 * OFMK_F_PARTIAL_COUNTS and the tile-order flags are ignored.  Argument checks: those of the ofmk_warp counterparts. */
typedef struct ofmk_affine { int64_t ayy, ayx, by, axy, axx, bx; } ofmk_affine;
int ofmk_affine_units(int h, int w, int H, int W, const ofmk_affine *geom, int out[5]);
int ofmk_warp_affine_rgb8(const uint8_t *in, int n, int h, int w, uint8_t *out, int Hout, int Wout, int oy, int ox,
                          const ofmk_affine *geom, void *stream, const ofmk_opts *opts);
int ofmk_svd_affine_scores_rgb8(const uint8_t *in, int n, int h, int w, int H, int W, const ofmk_affine *cands, int K,
                                const double *scales, int blk, long long *scores, void *stream, const ofmk_opts *opts);
int ofmk_svd_affine_phase_scores_rgb8(const uint8_t *in, int n, int h, int w, int H, int W, const ofmk_affine *cands, int K,
                                      const double *scales, int blk, long long *scores, long long *units, void *stream,
                                      const ofmk_opts *opts);
int ofmk_svd_detect_soft_affine_rgb8(const uint8_t *in, int n, int h, int w, int H, int W, const ofmk_affine *geom, int L,
                                     const double *scales, int blk, long long *soft, void *stream, const ofmk_opts *opts);

/* ---- reading a leak against its SOURCE frames: the sums of a registration step (BUILD EXTENSION) -------------------------------
 * The operator who reads a leak holds the frames it was made from, so the leak's geometry can be fitted to them -- six parameters,
 * Gauss-Newton on the luma difference, coarse to fine (offmark.resync.register_leak) -- and needs no list.  Interleaved u8 RGB; the
 * codec takes no part.  Everything is an integer, so the device equals the NumPy statement (tests/_align.py) integer for integer.
 *
 *   Y = (R + 2*G + B + 2) >> 2, in 0..255.  T = Y of the source frame on the canvas H x W; Yw = Y of the bytes
 *   ofmk_warp_affine_rgb8 gives for the leak frame under the geometry (ofmk_affine's rule, unchanged).
 *       gy = T[y+1][x] - T[y-1][x]      gx = T[y][x+1] - T[y][x-1]                (twice the derivative)
 *   Canvas pixel (y, x) CONTRIBUTES iff 1 <= y <= H-2, 1 <= x <= W-2 and it is inside the leak by ofmk_affine's rule.  With
 *       yc = y - (H >> 1)    xc = x - (W >> 1)    sd = (gy*yc, gy*xc, gy, gx*yc, gx*xc, gx)    e = Yw - T
 *   the 29 sums over the contributing pixels are
 *       [0..20]  the upper triangle of sum sd sd^T, row-major (i <= j)      [21..26]  sum sd*e
 *       [27]     sum e*e                                                     [28]      the number of contributing pixels
 *   Overflow: H, W <= 4096 is required (else OFMK_E_ARG), so |sd| <= 255 * 2048 < 2^19, a product is below 2^38 and a frame has at
 *   most 2^24 pixels: every sum of one frame stays below 2^62.  Sums of several frames are added by the caller (Python integers).
 *
 * ofmk_align_sums_rgb8: src is device u8 [n][H][W][3], src[f] the source of leak frame f; leak is device u8 [n][h][w][3]; cands is
 *   DEVICE memory, ofmk_affine [K]; sums is device int64 [n][K][29], cleared by the call whatever it held.  A candidate out of
 *   ofmk_affine's range leaves 29 zeros (the list is not read on the host).  A workgroup owns a tile of 64 x 64 canvas pixels of one
 *   candidate and one frame and leaves at once when the tile lies wholly beyond one edge of the leak; the warped taps are formed as
 *   in ofmk_svd_affine_scores_rgb8 and no warped frame is written; partial sums stay in registers, then wavefront, LDS and at most
 *   29 64-bit atomics per workgroup -- integer adds, so the result does not depend on their order.  Candidates in gridDim.y and
 *   frames in gridDim.z, chunked at 65535 and below 2^30 workgroups per launch.  Byte loads of src; no alignment is assumed.
 *   Required, else OFMK_E_ARG: n >= 1, 8 <= H, W <= 4096, h, w >= 1 with h*w < 2^28, K >= 1, n*K < 2^40, no null pointer.
 * ofmk_halve_rgb8: the pyramid's 2x2 box, out[Y][X][c] = (in[2Y][2X][c] + in[2Y][2X+1][c] + in[2Y+1][2X][c] + in[2Y+1][2X+1][c] + 2) >> 2,
 *   device u8 [n][h/2][w/2][3], every byte written; an odd last row or column of the input is dropped.  Level l+1 pixel P sits at
 *   level-l coordinate 2P + 1/2, for canvas and leak alike, so a geometry keeps its linear part between levels and its offsets
 *   follow offmark.resync.level_down / level_up.  Required, else OFMK_E_ARG: n >= 1, h*w < 2^28, h/2 >= 8 and w/2 >= 8.
 * Both calls allocate nothing, synchronise nothing and are graph capturable; both are timed as kind 4 (svd); the flags are ignored. */
int ofmk_align_sums_rgb8(const uint8_t *src, const uint8_t *leak, int n, int h, int w, int H, int W, const ofmk_affine *cands, int K,
                         long long *sums, void *stream, const ofmk_opts *opts);
int ofmk_halve_rgb8(const uint8_t *in, int n, int h, int w, uint8_t *out, void *stream, const ofmk_opts *opts);

/* ---- matching the frames of a leaked CLIP to the frames of its source video (BUILD EXTENSION) ---------------------------------
 * A leak is a clip: it starts somewhere in the video, and a frame-rate conversion has dropped or doubled frames.  Which source frame
 * a leak frame came from is found in two passes (offmark.temporal): a coarse one on 8 x 8 luma thumbnails, and an exact one on the
 * luma residual at the registered geometry.  Interleaved u8 RGB; the codec takes no part.  Everything is an integer, so the device
 * equals the NumPy statement (tests/_temporal.py) byte for byte.  Y = (R + 2*G + B + 2) >> 2 as above.
 *
 * ofmk_signature_rgb8: in is device u8 [n][h][w][3]; sig is device u8 [n][64], every byte written.  Cell (i, j), 0 <= i, j < 8,
 *   covers rows (i*h) >> 3 .. ((i+1)*h) >> 3 - 1 and columns (j*w) >> 3 .. ((j+1)*w) >> 3 - 1; with A its area,
 *       sig[f][8*i + j] = (2 * sum Y + A) / (2 * A)                                 (the rounded mean, halves up, 0..255)
 *   A workgroup per frame and row of cells, frames in gridDim.x (no chunking).  No alignment is assumed: four pixels are fetched as
 *   three dwords at any address, the columns past the last group of four with byte loads; no load leaves the frame.
 *   Required, else OFMK_E_ARG: n >= 1, h, w >= 8, h*w < 2^28, no null pointer.
 * ofmk_signature_distances: a is device u8 [m][64], b device u8 [N][64]; dist is device int32 [m][N], every entry written:
 *       dist[i][t] = sum over c < 64 of |a[i][c] - b[t][c]|                         (at most 16320)
 *   A thread keeps one row of b in 16 registers, 32 rows of a sit in LDS, four bytes per v_sad_u8, stores coalesced along N.
 *   Required, else OFMK_E_ARG: m, N >= 1, m*N < 2^40, no null pointer.
 * ofmk_align_residuals_rgb8: lib is device u8 [N][H][W][3], the source frames; leak is device u8 [m][h][w][3]; first is DEVICE int32
 *   [m]; geom is ONE geometry in HOST memory (ofmk_affine's rules, else OFMK_E_ARG); res is device int64 [m][span][2], cleared by the
 *   call whatever it held.  With s = first[i] + j, res[i][j] = (sum e*e, the number of contributing pixels): entries [27] and [28] of
 *   ofmk_align_sums_rgb8 for source lib[s] and leak frame i under geom -- the same contributing-pixel rule, the same warp.  s
 *   outside 0..N-1 leaves (0, 0); the list is not read on the host.  A workgroup owns a tile of 64 x 64 canvas pixels of one leak
 *   frame: it forms the warped luma of its pixels once, then walks the span sources reading only their luma; each source's squares
 *   are reduced in 32 bits (a tile's stay below 2^29), then at most 2*span 64-bit atomics per workgroup -- integer adds, so the order
 *   is free.  No warped frame and no gathered source is written.  Leak frames in gridDim.y, chunked at 65535.
 *   Required, else OFMK_E_ARG: m, N >= 1, 1 <= span <= 16, 8 <= H, W <= 4096, h, w >= 1 with h*w < 2^28, no null pointer.
 * The three calls allocate nothing, synchronise nothing and are graph capturable; all are timed as kind 4 (svd); the flags are
 * ignored. */
int ofmk_signature_rgb8(const uint8_t *in, int n, int h, int w, uint8_t *sig, void *stream, const ofmk_opts *opts);
int ofmk_signature_distances(const uint8_t *a, int m, const uint8_t *b, int N, int32_t *dist, void *stream, const ofmk_opts *opts);
int ofmk_align_residuals_rgb8(const uint8_t *lib, int N, const uint8_t *leak, int m, int h, int w, int H, int W, const int32_t *first,
                              int span, const ofmk_affine *geom, long long *res, void *stream, const ofmk_opts *opts);

/* ---- a leaked clip whose TONE changed as well: tone-invariant frame matching (BUILD EXTENSION) -----------------------------------
 * A re-graded or screen-captured clip is both a clip (above) and a leak whose values changed (below).  In a dissolve brightness is
 * time, so the plain signature loses its strongest cue, and sum e*e moves more with a gain than with a wrong frame.  Two calls make
 * the two passes of offmark.temporal tone invariant (offmark.temporal.read_toned_leak_clip); all integers, equal to the NumPy
 * statement (tests/_toned_clip.py).
 *
 * ofmk_align_moments_rgb8: the arguments of ofmk_align_residuals_rgb8, their rules and its OFMK_E_ARG cases; mom is device int64
 *   [m][span][6], cleared by the call whatever it held.  With l the warped luma of leak frame i under geom, s the luma of
 *   lib[first[i] + j] and the sums over ofmk_align_sums_rgb8's contributing pixels (interior canvas pixels inside the leak):
 *       mom[i][j] = (count, sum l, sum s, sum l*l, sum s*s, sum l*s)
 *   A source index outside 0..N-1 leaves six zeros; the list is not read on the host.  mom[3] + mom[4] - 2*mom[5] equals
 *   ofmk_align_residuals_rgb8's sum e*e and mom[0] its count, integer for integer.  The zero-mean normalised cross-correlation they
 *   give (offmark.temporal.ncc_cost) does not see a gain or an offset on either side.  ofmk_align_residuals_rgb8's workgroup: a tile of
 *   64 x 64 canvas pixels of one leak frame, the warped luma formed once and kept in registers, then the span sources, reading only
 *   their luma; per source three sums reduced in 32 bits (a tile's sum s*s, sum l*l, sum l*s stay below 4096 * 255^2 < 2^29, sum l
 *   and sum s below 2^20): wavefront, LDS, then at most 6*span 64-bit atomics per workgroup -- integer adds, so the order is free.
 *   No warped frame and no gathered source is written.  Leak frames in gridDim.y, chunked at 65535.
 * ofmk_signature_ranks: sig is device u8 [n][64] (ofmk_signature_rgb8's); rank is device u8 [n][64], every byte written:
 *       rank[f][c] = the number of c' < 64 with (sig[f][c'], c') < (sig[f][c], c)     (pairs compared in order: value, then index)
 *   a permutation of 0..63 per frame, which any increasing tone curve leaves unchanged; ofmk_signature_distances runs on ranks as it
 *   does on signatures (at most 2048).  One wavefront per frame, a lane per cell, the 64 keys read lane by lane; no LDS.
 *   Required, else OFMK_E_ARG: n >= 1, no null pointer.
 * Both calls allocate nothing, synchronise nothing and are graph capturable; both are timed as kind 4 (svd); the flags are ignored. */
int ofmk_align_moments_rgb8(const uint8_t *lib, int N, const uint8_t *leak, int m, int h, int w, int H, int W, const int32_t *first,
                            int span, const ofmk_affine *geom, long long *mom, void *stream, const ofmk_opts *opts);
int ofmk_signature_ranks(const uint8_t *sig, int n, uint8_t *rank, void *stream, const ofmk_opts *opts);

/* ---- reading a leak whose VALUES changed: a tone curve fitted against the SOURCE frames (BUILD EXTENSION) ----------------------
 * A screen capture, a re-grade or a range mix-up changes a leak's brightness, contrast or gamma, and the DwtDctSvd mark -- the place
 * of a singular value inside a cell 15 wide -- does not survive a gain of a few percent.  The operator holds the source frames, so the
 * per-channel curve that takes the leak's values back to the source's can be fitted to them (offmark.tone.read_toned_leak), as the
 * geometry is: a histogram match for a first registration, then the mean source value per leak value under the registered geometry.
 * Interleaved u8 RGB; the codec takes no part.  Everything is an integer, so the device equals the NumPy statement (tests/_tone.py)
 * exactly.
 *
 * ofmk_histograms_rgb8: in is device u8 [n][h][w][3]; hist is device int64 [n][3][256], cleared by the call whatever it held:
 *       hist[f][c][v] = the number of pixels of frame f whose channel c equals v
 *   Four pixels are fetched as three dwords at any address, the pixels past the last group of four with byte loads; no load leaves
 *   the frame and no alignment is assumed.  A workgroup counts 16384 pixels into a table in LDS, eight copies of it so that the lanes of
 *   a wavefront that meet in one bin (flat content) spread over eight words, then adds its non-zero bins with 64-bit atomics.
 *   Frames in gridDim.y, chunked at 65535.  Required, else OFMK_E_ARG: n >= 1, h, w >= 1 with h*w < 2^28, no null pointer.
 * ofmk_tone_sums_rgb8: the arguments of ofmk_align_sums_rgb8 -- src is device u8 [n][H][W][3], src[f] the source of leak frame f;
 *   leak is device u8 [n][h][w][3]; cands is DEVICE memory, ofmk_affine [K] -- and sums is device int64 [n][K][3][256][2], cleared by
 *   the call whatever it held.  Canvas pixel (y, x) contributes iff it is inside the leak by ofmk_affine's per-pixel rule (no border
 *   is left out).  With v the byte ofmk_warp_affine_rgb8 would write at (y, x, c) under cands[k]:
 *       sums[f][k][c][v][0] += 1          sums[f][k][c][v][1] += src[f][y][x][c]
 *   A candidate out of ofmk_affine's range leaves zeros (the list is not read on the host).  A workgroup owns a tile of 64 x 64
 *   canvas pixels of one candidate and one frame and leaves at once when the tile lies wholly beyond one edge of the leak; the taps
 *   are formed as in ofmk_align_sums_rgb8 and no warped frame is written.  It accumulates into a table of 3*256*2 32-bit words in
 *   LDS (a tile's entries stay below 4096 * 255 < 2^20): a lane adds a run of equal values down its column once, and a wavefront
 *   whose lanes all add to one bin adds once; then the bins with a count go to sums with 64-bit atomics -- integer adds, so the
 *   result does not depend on their order.  Candidates in gridDim.y and frames in gridDim.z, chunked at 65535 and below 2^30
 *   workgroups per launch.  Required, else OFMK_E_ARG: n >= 1, 8 <= H, W <= 4096, h, w >= 1 with h*w < 2^28, K >= 1, n*K < 2^40,
 *   no null pointer.
 * ofmk_apply_tone_rgb8: in is device u8 [n][h][w][3]; lut is DEVICE u8 [3][256]; out is device u8 [n][h][w][3], every byte written:
 *       out[f][y][x][c] = lut[c][in[f][y][x][c]]
 *   out == in (exactly) is allowed; any other overlap is not.  12 bytes per thread as three dwords at any address, in and out; no
 *   alignment is assumed.  Required, else OFMK_E_ARG: n >= 1, h, w >= 1 with h*w < 2^28, no null pointer.
 * The three calls allocate nothing, synchronise nothing and are graph capturable; all are timed as kind 4 (svd); the flags are
 * ignored. */
int ofmk_histograms_rgb8(const uint8_t *in, int n, int h, int w, long long *hist, void *stream, const ofmk_opts *opts);
int ofmk_tone_sums_rgb8(const uint8_t *src, const uint8_t *leak, int n, int h, int w, int H, int W, const ofmk_affine *cands, int K,
                        long long *sums, void *stream, const ofmk_opts *opts);
int ofmk_apply_tone_rgb8(const uint8_t *in, int n, int h, int w, const uint8_t *lut, uint8_t *out, void *stream, const ofmk_opts *opts);

/* ---- reading a leak whose COLOURS changed: a matrix fitted against the SOURCE frames (BUILD EXTENSION) --------------------------
 * A BT.601 / BT.709 mix-up, a saturation setting or a hue shift is a 3 x 3 matrix plus an offset on RGB.  No per-channel curve undoes
 * a matrix, and the DwtDctSvd mark lives in U, a difference of channels: it leaves its cell 15 wide as soon as the channels mix.  The
 * operator holds the source frames, so the matrix that takes the leak's pixels back to the source's is fitted to them by least squares
 * (offmark.colour.read_coloured_leak), as the tone curve is: a histogram match for a first registration, then the sums below under
 * the registered geometry, an exact solve on the host, and the matrix applied in integers.  Interleaved u8 RGB; the codec takes no
 * part.  Everything is an integer, so the device equals the NumPy statement (tests/_colour.py) exactly.
 *
 * ofmk_colour_sums_rgb8: the arguments of ofmk_tone_sums_rgb8 -- src is device u8 [n][H][W][3], src[f] the source of leak frame f;
 *   leak is device u8 [n][h][w][3]; cands is DEVICE memory, ofmk_affine [K] -- and sums is device int64 [n][K][28], cleared by the call
 *   whatever it held.  Canvas pixel (y, x) contributes iff it is inside the leak by ofmk_affine's per-pixel rule (no border is left
 *   out) AND the three bytes l that ofmk_warp_affine_rgb8 would write there under cands[k] all lie in 1..254: a clipped pixel says
 *   nothing about the matrix and bends the fit.  With s = src[f][y][x]:
 *       sums[f][k][0] += 1      sums[f][k][1 + c] += l[c]      sums[f][k][4 + c] += s[c]
 *       sums[f][k][7..12] += l[i] * l[j]      sums[f][k][13..18] += s[i] * s[j]      for (i, j) = (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
 *       sums[f][k][19 + 3 * i + j] += l[i] * s[j]
 *   the normal equations of s ~ M l + t and what its residual needs.  A candidate out of ofmk_affine's range leaves 28 zeros (the list
 *   is not read on the host).  A workgroup owns a tile of 64 x 64 canvas pixels of one candidate and one frame and leaves at once when
 *   the tile lies wholly beyond one edge of the leak; the taps are formed as in ofmk_align_sums_rgb8 and no warped frame is written.
 *   28 sums per thread in registers, then the wavefront and LDS in 32 unsigned bits (a tile's sums stay below 4096 * 255^2 < 2^28),
 *   then at most 28 64-bit atomics per workgroup -- integer adds, so the result does not depend on their order.  Candidates in
 *   gridDim.y and frames in gridDim.z, chunked at 65535 and below 2^30 workgroups per launch.  Required, else OFMK_E_ARG: n >= 1,
 *   8 <= H, W <= 4096, h, w >= 1 with h*w < 2^28, K >= 1, n*K < 2^40, no null pointer.
 * ofmk_apply_colour_rgb8: in is device u8 [n][h][w][3]; matrix is HOST int32 [3][4] in Q16, row c the three coefficients and then the
 *   offset, read by the call and handed to the kernel by value; out is device u8 [n][h][w][3], every byte written:
 *       out[f][y][x][c] = clip((m[c][0] * in[0] + m[c][1] * in[1] + m[c][2] * in[2] + m[c][3] + 32768) >> 16, 0, 255)
 *   with in[.] the three bytes of in[f][y][x] and an arithmetic shift.  |coefficient| <= 2^21 and |offset| <= 2^28, else OFMK_E_ARG:
 *   the sum then stays inside int32.  out == in (exactly) is allowed; any other overlap is not.  12 bytes = four pixels per thread as
 *   three dwords at any address, in and out; no alignment is assumed.  Required, else OFMK_E_ARG: n >= 1, h, w >= 1 with h*w < 2^28,
 *   no null pointer, a matrix in range.
 * Both calls allocate nothing, synchronise nothing and are graph capturable (a captured ofmk_apply_colour_rgb8 keeps the matrix it was
 * captured with); both are timed as kind 4 (svd); the flags are ignored. */
int ofmk_colour_sums_rgb8(const uint8_t *src, const uint8_t *leak, int n, int h, int w, int H, int W, const ofmk_affine *cands, int K,
                          long long *sums, void *stream, const ofmk_opts *opts);
int ofmk_apply_colour_rgb8(const uint8_t *in, int n, int h, int w, const int32_t *matrix /* HOST, [3][4] */, uint8_t *out, void *stream,
                           const ofmk_opts *opts);

/* ---- DeShuffler.degenerate's epilogue for a batch, on the device ---------------------------
 * src/offmark/degenerator/de_shuffler.py:17-22: mean of bits[i::L] (from `counts`), undo the key
 * permutation (`perm` = DeShuffler.payload_idx, device int32 [L]), threshold strictly above the
 * mid-range of the L means.  payload: device u8 [n][L].  n_bits = H*W/64.                   */
int ofmk_payloads_from_counts(const int32_t *counts, int n, int L, int n_bits, const int32_t *perm,
                              uint8_t *payload, void *stream, const ofmk_opts *opts);
/* Rows of a frame's partial counts (OFMK_F_PARTIAL_COUNTS) for the DwtDctSvd codec with this blk; negative on bad arguments. */
int ofmk_svd_count_tiles(int H, int W, int blk);
/* The payload epilogue from partial counts [n][tiles][L] (OFMK_F_PARTIAL_COUNTS): per frame, counts[i] = sum over tiles, then
 * exactly ofmk_payloads_from_counts (de_shuffler.py:17-22).  payload: device u8 [n][L] or NULL; counts: device int32 [n][L]
 * or NULL (the summed counts, for callers that want DeShuffler's numerators); at least one of the two.  L <= 2048. */
int ofmk_payloads_from_partial_counts(const int32_t *partials, int tiles, int n, int L, int n_bits, const int32_t *perm,
                                      uint8_t *payload, int32_t *counts, void *stream, const ofmk_opts *opts);

/* ---- plugin-level entry points on float32 YUV frames --------------------------------------
 * DctEncoder.encode(yuv) (dct_encoder.py:18-39; mutates channel 1 in place) and
 * DctDecoder.decode(yuv) (dct_decoder.py:10-27).  yuv: device f32 [n][H][W][3].            */
int ofmk_encode_yuv32f(float *yuv, int n, int H, int W,
                       const uint8_t *wm, int n_wm, const int32_t *wm_row, double alpha,
                       int chunk_frames, void *workspace, size_t workspace_bytes, void *stream,
                       const ofmk_opts *opts);
int ofmk_decode_yuv32f(const float *yuv, int n, int H, int W, int L, double alpha,
                       int32_t *counts, uint8_t *bits,
                       int chunk_frames, void *workspace, size_t workspace_bytes, void *stream,
                       const ofmk_opts *opts);

/* ---- parity / debug planes for ONE frame (any pointer may be NULL) -----------------------
 * DctEncoder.luminance_mask / texture_mask (dct_encoder.py:41-102) and the [2][1] coefficient
 * before and after quantisation (dct_encoder.py:29-35).  All planes are [H/8][W/8].
 *   src_is_yuv32f = 0: frame is u8 [H][W][3];  1: frame is f32 YUV [H][W][3]
 *   wm may be NULL (then c21_post is not produced)                                          */
int ofmk_debug_planes(const void *frame, int src_is_yuv32f, int H, int W, double alpha,
                      const uint8_t *wm,
                      float *y_dc, double *lum_mask, double *tex_mask, double *step,
                      float *c21_pre, float *c21_post,
                      void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts);

/* ---- individual stages (bench.py and tests drive single kernels with these) ----------------
 * analyze : frames -> per-block records (the kernel shared by embed and detect)
 * mark    : frames + the records the analyze stage left in the workspace for the SAME frames +
 *           watermark (row 0 for every frame) -> marked frames; fused != 0 also analyzes the
 *           marked frames (mark + verify kernel)                                             */
int ofmk_stage_analyze_rgb8(const uint8_t *in, int n, int H, int W,
                            void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts);
int ofmk_stage_mark_rgb8(const uint8_t *in, uint8_t *out, int n, int H, int W,
                         const uint8_t *wm, double alpha, int fused,
                         void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts);

/* Streaming probes: bench.py measures the device's achievable HBM rates with them in the same run as the
 * kernels.  ofmk_hbm_copy: device-to-device copy, 16 bytes per lane and access, registers only (reads `bytes`,
 * writes `bytes`).  ofmk_hbm_read: read-only stream of `bytes`; `sink` is a device uint32 the kernel
 * practically never writes (it only keeps the loads alive). */
int ofmk_hbm_copy(const void *src, void *dst, size_t bytes, void *stream);
int ofmk_hbm_read(const void *src, size_t bytes, void *sink, void *stream);

/* Which XCD each workgroup of a linear grid of `n_workgroups` 64-thread workgroups runs on (HW_REG_XCC_ID): device int32
 * [n_workgroups].  HIP promises nothing about that deal; the XCD-aware tile order assumes workgroups L and L + xcds share an
 * XCD (speed only, never correctness), and this lets a host check it and count the XCDs (bench.py: `mark_order.xcc_deal`). */
int ofmk_probe_xcc(int32_t *xcc_of_workgroup, int n_workgroups, void *stream, const ofmk_opts *opts);

/* Per-launch HIP-event timing for bench.py.  A timing object owns 2*max_launches events; while it is passed in
 * ofmk_opts.timing every launch of a kernel kind selected in kind_mask (bit k = kind k, 0 = all) carries an event
 * pair as the dispatch's own start/stop events (hipExtLaunchKernelGGL) on the launch stream, so no marker packets
 * separate consecutive kernels.  collect() waits for the recorded events, returns the summed milliseconds and
 * launch counts per kernel kind (0 analyze, 1 finalize, 2 mark, 3 fused mark+analyze, 4 DwtDctSvd, 5 planar 4:2:0
 * analyze, 6 planar 4:2:0 mark) and rewinds the pool.  One object per engine / host thread; a call that carries one cannot be
 * captured into a hipGraph (events on the dispatch). */
#define OFMK_TIMING_KINDS 7
int ofmk_timing_create(int max_launches, unsigned kind_mask, ofmk_timing **out);
int ofmk_timing_collect(ofmk_timing *t, double *ms_by_kind /*[OFMK_TIMING_KINDS]*/, int *launches_by_kind /*[OFMK_TIMING_KINDS]*/);
/* The recorded launches one by one, in launch order (waits for their events; does NOT rewind the pool: call before collect):
 * duration in ms and kernel kind of up to `cap` launches.  Returns the number written, or a negative error code.  bench.py
 * uses it to show how the dominant kernel's duration moves through the timed region (clock ramp after idle). */
int ofmk_timing_durations(ofmk_timing *t, float *ms_per_launch, int *kind_per_launch /* may be NULL */, int cap);
void ofmk_timing_destroy(ofmk_timing *t);

#ifdef __cplusplus
}
#endif
#endif /* OFFMARK_HIP_H */
