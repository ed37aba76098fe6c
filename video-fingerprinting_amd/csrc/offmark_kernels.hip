// offmark_kernels.hip -- hand-written gfx950 (MI355X / CDNA4) kernels + C ABI for the offmark
// DCT frame-watermark path.  Built with:
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize
//
// Reference behaviour restated here (paths relative to the reference root):
//   src/offmark/video/embedder.py:33-39      u8 -> f32 -> "BGR2YUV" -> encode -> "YUV2BGR" -> clip/round/u8
//   src/offmark/embed/dct_encoder.py:18-102  masks from the Y block DCTs, QIM on U coefficient [2][1]
//   src/offmark/extract/dct_decoder.py:10-27 same masks, bit = round(c21/step) odd
//   src/offmark/degenerator/de_shuffler.py:17-18  sums of bits[i::L] (the mean's numerator)
//
// Kernels (DESIGN.md has the full story):
//   analyze  : frame pixels -> 3 floats per 8x8 block {A00, texture-mask code, C21} + a fixed-point
//              sum of the block DCs (the luminance mask needs the frame-global mean first).
//              Shared by embed and detect.  Reads 3 B/px, writes 0.19 B/px.
//   finalize : one thread per block: luminance mask (float64 like the reference), step, then
//              either the QIM delta of C21 (embed) or the read-out bit + bits[i::L] counts.
//   mark     : frame pixels + delta -> marked pixels.  The 8x8 DCT is orthonormal, so
//              idct(dct(U) + d*e21) == U + d * outer(c2, c1): a rank-1 update, no DCT needed.
//              The FUSED variant also analyzes the marked block it has just produced (mark +
//              verify), which saves detect's read of the marked frame.
//
// Work decomposition: ONE THREAD PER 8x8 BLOCK.  A lane owns 8 rows x 24 contiguous bytes; the 64
// lanes of a wavefront own 64 adjacent blocks, so every row load of a wave covers 1536 contiguous
// bytes.  Row DCTs, column DCTs and all per-block sums stay in that lane's registers: no LDS, no
// barrier, no cross-lane traffic.  (A first version staged the 8x8 transpose through LDS with
// 8-lane DPP sums; rocprofv3 showed VALU ~58 % and the LDS pipe ~55 % busy at once -- see
// profiles/ -- and this form needs ~20 % fewer VALU instructions and none of the LDS ones.)
// It also lets the texture-feature sums follow numpy's exact association order.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "../../include/offmark_hip.h"

#include "common.hiph"
#include "readout.hiph"
#include "dct_kernels.hiph"
#include "svd_kernels.hiph"
#include "svd8_kernels.hiph"
#include "misc_kernels.hiph"
#include "planar_kernels.hiph"
#include "svd_planar_kernels.hiph"
#include "copies_kernels.hiph"
#include "planar_copies_kernels.hiph"
#include "resync_kernels.hiph"
#include "dct_resync_kernels.hiph"
#include "planar_resync_kernels.hiph"
#include "warp_kernels.hiph"
#include "affine_kernels.hiph"
#include "affine_phase_kernels.hiph"
#include "align_kernels.hiph"
#include "temporal_kernels.hiph"
#include "tone_kernels.hiph"
#include "colour_kernels.hiph"

namespace {

using namespace ofmk;

// ------------------------------------------------------------------------------------------
// host side of the C ABI
// ------------------------------------------------------------------------------------------
thread_local char g_err[512] = "";     // the ONLY mutable state of the library: the calling thread's last error text

// Optional per-launch HIP-event timing (bench.py).  The event pool is an object the CALLER owns
// (ofmk_timing_create) and passes in ofmk_opts; no library-wide state.
enum { KIND_ANALYZE = 0, KIND_FINALIZE = 1, KIND_MARK = 2, KIND_MARK_FUSED = 3, KIND_SVD = 4, KIND_PLANAR_ANALYZE = 5, KIND_PLANAR_MARK = 6, KIND_COUNT = 7 };
static_assert(KIND_COUNT == OFMK_TIMING_KINDS, "timing kinds");
struct TimingRec { hipEvent_t a, b; int kind; };

}  // namespace

struct ofmk_timing {
    TimingRec *rec;
    int cap;
    std::atomic<int> used;      // launches that took a pair; may exceed cap (then the surplus launches go untimed)
    unsigned mask;              // which kernel kinds get an event pair
};

namespace {

// What a launcher needs besides its operands: the stream and the (optional) event pool of this call.
struct Ctx {
    hipStream_t s;
    ofmk_timing *t;
    unsigned flags;
    int xcds;         // XCDs the XCD-aware tile order assumes (common.hiph: xcd_tile); which order a launch uses: tile_xcds()
};
constexpr int kDefaultXcds = 8;      // MI355X in SPX mode; ofmk_opts.xcds overrides (ofmk_probe_xcc counts the real ones)
Ctx make_ctx(void *stream, const ofmk_opts *o) {
    Ctx c;
    c.s = static_cast<hipStream_t>(stream);
    c.t = o ? o->timing : nullptr;
    c.flags = o ? o->flags : 0u;
    c.xcds = o && o->xcds ? (int)o->xcds : kDefaultXcds;
    if (c.xcds == 1) c.xcds = 0;
    return c;
}

// Tile order of one launch of the frame-writing DCT kernel (include/offmark_hip.h: OFMK_F_LINEAR_TILES / OFMK_F_XCD_TILES).
// Without a flag the library decides by a STATIC rule on the bytes of frames the launch reads: XCD-aware from
// OFMK_XCD_TILES_MIN_BYTES (192 frames of 1080p) up, linear below.  That is what every interleaved A/B since round 3 says
// (profiles/r4_mark_fused_pass.txt, r4_bench_config4.json, r6_mark_ladder.txt): at 300-384 x 1080p per launch the XCD-aware order
// wins by 1.5-7 % or ties, depending on where the driver placed the caller's frames; at 192 frames the two tie; at 48-96 frames
// linear wins by 1-4 %.  Nothing is measured at run time (rounds 4-5 carried a calibration mode in the Python engine; removed).
int tile_xcds(const Ctx &cx, size_t frame_bytes_per_launch) {
    if (cx.flags & OFMK_F_LINEAR_TILES) return 0;
    if (cx.flags & OFMK_F_XCD_TILES) return cx.xcds;
    return frame_bytes_per_launch >= (size_t)OFMK_XCD_TILES_MIN_BYTES ? cx.xcds : 0;
}

struct ScopedTiming {      // reserves an event pair for the launch that follows (none when timing is off)
    TimingRec *r;
    ScopedTiming(int kind, const Ctx &c) : r(nullptr) {
        if (c.t && ((c.t->mask >> kind) & 1u)) {
            const int k = c.t->used.fetch_add(1, std::memory_order_relaxed);
            if (k < c.t->cap) {
                r = &c.t->rec[k];
                r->kind = kind;
            }
        }
    }
};
// A timed launch hands its event pair to the dispatch itself (hipExtLaunchKernelGGL): the events take the
// kernel's own begin/end timestamps and no marker packets go into the stream, so consecutive kernels still
// dispatch back to back (bracketing with hipEventRecord cost 3-7 % of throughput).
#define OFMK_TIMED_LAUNCH(T, KERNEL, GRID, BLOCK, SHMEM, STREAM, ...)                                            \
    do {                                                                                                         \
        if ((T).r) hipExtLaunchKernelGGL(KERNEL, GRID, BLOCK, SHMEM, STREAM, (T).r->a, (T).r->b, 0, __VA_ARGS__); \
        else hipLaunchKernelGGL(KERNEL, GRID, BLOCK, SHMEM, STREAM, __VA_ARGS__);                                \
    } while (0)

int fail(int code, const char *fmt, const char *detail = "") {
    snprintf(g_err, sizeof(g_err), fmt, detail);
    return code;
}
#define HIP_TRY(expr)                                                                    \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) return fail(OFMK_E_HIP, #expr ": %s", hipGetErrorString(e_)); \
    } while (0)

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Zero-fill as a KERNEL, never hipMemsetAsync: every compute call must replay correctly from a captured hipGraph, and on ROCm 7.2
// a graph that holds memset node -> kernel nodes -> memset node OF THE SAME BUFFER -> kernel nodes (two steps of a call sequence
// sharing one counts / accumulator buffer) replays with the memsets out of order from the second replay on: measured with
// tools/graph_memset_order.py (payloads right on the first replay, wrong on every later one; distinct buffers or this kernel: always
// right); tests/test_gpu_parity.py::test_several_steps_in_one_graph_replay_like_eager pins it for both codecs.
hipError_t launch_zero(void *p, size_t bytes, hipStream_t s) {
    if (bytes == 0) return hipSuccess;
    const size_t vec = bytes / 16 + 1;
    const unsigned grid = (unsigned)(vec < 256 * 2048 ? (vec + 255) / 256 : 2048);
    hipLaunchKernelGGL(zero_kernel, dim3(grid), dim3(256), 0, s, static_cast<uint8_t *>(p), bytes);
    return hipGetLastError();
}

constexpr int kMaxChunk = 65535;   // frames per launch = gridDim.y

// Frames [0, n) in chunks of at most cap (a workspace's capacity, or kMaxChunk): body(f0, cf) for frames [f0, f0 + cf), until
// one returns an error code.
template <class Body>
int for_chunks(int n, int cap, Body &&body) {
    for (int f0 = 0; f0 < n; f0 += cap)
        if (int rc = body(f0, n - f0 < cap ? n - f0 : cap)) return rc;
    return OFMK_OK;
}

// Runtime flag -> template argument: f is a generic lambda that receives the value as a std::integral_constant and names the kernel
// instantiation with decltype(arg)::value.  Only the combinations a call site spells out get instantiated.
template <class F>
void with_bool(bool b, F &&f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
template <class F>
void with_fmt(int layout, F &&f) {       // OFMK_YUV_I420 / OFMK_YUV_NV12 -> FMT_I420 / FMT_NV12 (planar_kernels.hiph)
    if (layout == OFMK_YUV_I420) f(std::integral_constant<int, FMT_I420>{});
    else f(std::integral_constant<int, FMT_NV12>{});
}
// f(mode, multi) of the DwtDctSvd frame kernels; the read-out alone (hard or soft) has no MULTI = true form.
template <class F>
void with_svd_mode(int mode, bool multi, F &&f) {
    if (mode == SVD_DETECT) f(std::integral_constant<int, SVD_DETECT>{}, std::false_type{});
    else if (mode == SVD_DETECT_SOFT) f(std::integral_constant<int, SVD_DETECT_SOFT>{}, std::false_type{});
    else if (mode == SVD_EMBED) with_bool(multi, [&](auto mu) { f(std::integral_constant<int, SVD_EMBED>{}, mu); });
    else with_bool(multi, [&](auto mu) { f(std::integral_constant<int, SVD_EMBED_VERIFY>{}, mu); });
}

struct Workspace {
    float *rec;      // kRec planes of [frames][nblk]
    float *delta;    // [frames][nblk]
    unsigned long long *ysum;    // [frames][tiles] per-tile partial sums of the block DCs of the frames analyze() saw
    unsigned long long *ysum2;   // ... of the marked frames (fused mark+verify kernel)
    int frames;      // chunk capacity
    int tiles;       // workgroups per frame of the frame kernels
    size_t plane;    // frames * nblk
};

constexpr size_t kFixedBytes = 4096;     // alignment slack of the carved arrays

size_t tiles_per_frame(int H, int W) { return ((size_t)(H / 8) * (W / 8) + kThreads - 1) / kThreads; }

size_t per_frame_bytes(int H, int W) {
    const size_t nblk = (size_t)(H / 8) * (W / 8);
    return nblk * (kRec + 1) * sizeof(float) + 2 * tiles_per_frame(H, W) * 8;
}

int carve(void *ws, size_t bytes, int H, int W, int want_frames, Workspace &out) {
    if (!ws) return fail(OFMK_E_ARG, "workspace is null%s");
    if ((uintptr_t)ws % 256) return fail(OFMK_E_ARG, "workspace must be 256-byte aligned%s");
    const size_t per = per_frame_bytes(H, W);
    if (bytes < per + kFixedBytes) return fail(OFMK_E_WORKSPACE, "workspace smaller than ofmk_workspace_bytes(1, H, W)%s");
    size_t cap = (bytes - kFixedBytes) / per;
    if (want_frames > 0 && (size_t)want_frames < cap) cap = want_frames;
    if (cap > (size_t)kMaxChunk) cap = kMaxChunk;
    const size_t nblk = (size_t)(H / 8) * (W / 8);
    char *p = static_cast<char *>(ws);
    out.frames = (int)cap;
    out.tiles = (int)tiles_per_frame(H, W);
    out.plane = cap * nblk;
    out.rec = reinterpret_cast<float *>(p);
    p += align256(out.plane * kRec * sizeof(float));
    out.delta = reinterpret_cast<float *>(p);
    p += align256(out.plane * sizeof(float));
    out.ysum = reinterpret_cast<unsigned long long *>(p);
    p += align256(cap * out.tiles * 8);
    out.ysum2 = reinterpret_cast<unsigned long long *>(p);
    return OFMK_OK;
}

// every entry point that takes ofmk_opts: unknown flag bits or a non-zero reserved word are a caller bug, not a default
int check_opts(const ofmk_opts *o) {
    if (o && ((o->flags & ~(uint32_t)(OFMK_F_SEPARATE_DETECT | OFMK_F_LINEAR_TILES | OFMK_F_XCD_TILES | OFMK_F_PARTIAL_COUNTS)) || o->xcds > 64u))
        return fail(OFMK_E_ARG, "ofmk_opts: unknown flag bits or xcds > 64%s");
    if (o && (o->flags & OFMK_F_LINEAR_TILES) && (o->flags & OFMK_F_XCD_TILES))
        return fail(OFMK_E_ARG, "ofmk_opts: OFMK_F_LINEAR_TILES and OFMK_F_XCD_TILES exclude each other%s");
    return OFMK_OK;
}

int check_dims(int n, int H, int W) {
    if (n <= 0) return fail(OFMK_E_ARG, "n must be positive%s");
    if (H < 8 || W < 8) return fail(OFMK_E_ARG, "H and W must be at least 8%s");
    if ((long long)H * W >= (1LL << 28)) return fail(OFMK_E_ARG, "frame too large (H*W must be < 2^28)%s");
    return OFMK_OK;
}

int check_embed_args(const void *in, const void *out, int n, int H, int W, const uint8_t *wm, int n_wm) {
    int rc = check_dims(n, H, W);
    if (rc) return rc;
    if (!in || !out || !wm) return fail(OFMK_E_ARG, "null frame or watermark pointer%s");
    if (n_wm < 1) return fail(OFMK_E_ARG, "n_wm must be >= 1%s");
    return OFMK_OK;
}

int check_detect_args(const void *in, int n, int H, int W, int L, const int32_t *counts, const uint8_t *bits) {
    int rc = check_dims(n, H, W);
    if (rc) return rc;
    if (!in) return fail(OFMK_E_ARG, "null frame pointer%s");
    if (L < 1) return fail(OFMK_E_ARG, "payload length L must be >= 1%s");
    if (!counts && !bits) return fail(OFMK_E_ARG, "both outputs (counts, bits) are null%s");
    return OFMK_OK;
}

// the soft read-outs (both codecs): the hard read-out's checks, with the one int64 [n][L] output in place of counts / bits
int check_soft_args(const void *in, int n, int H, int W, int L, const long long *soft) {
    if (int rc = check_dims(n, H, W)) return rc;
    if (!in || !soft) return fail(OFMK_E_ARG, "null pointer%s");
    if (L < 1) return fail(OFMK_E_ARG, "payload length L must be >= 1%s");
    return OFMK_OK;
}

Geom make_geom(int H, int W, const Workspace &ws, int frames = 0, int xcds = 0) {
    Geom g;
    g.frames = frames;
    g.xcds = xcds;
    g.W = W;
    g.wb = W / 8;
    g.inv_wb = 1.0f / (float)g.wb;
    g.nblk = (H / 8) * (W / 8);
    g.frame_stride = (size_t)H * W * 3;
    g.plane = ws.plane;
    return g;
}

// 2-D grid, tiles x frames (at most kMaxChunk): the kernels that gain nothing from the XCD order
dim3 grid_2d(int units_per_frame, int n) { return dim3((unsigned)((units_per_frame + kThreads - 1) / kThreads), (unsigned)n); }

// Linear grid of the frame kernels (common.hiph: xcd_tile): tiles x frames workgroups, padded to a multiple of the XCD count
// the tile order assumes (xcds <= 1: linear order, no padding); the kernels take the frame count from their geometry argument.
dim3 xcd_grid(int blocks_per_frame, int n, int xcds = 0) {
    const unsigned tiles = (unsigned)((blocks_per_frame + kThreads - 1) / kThreads);
    const unsigned long long G = (unsigned long long)tiles * (unsigned)n;
    const unsigned long long X = xcds > 1 ? (unsigned long long)xcds : 1ull;
    return dim3((unsigned)(((G + X - 1) / X) * X));
}

bool aligned_rows(const void *p, int W, size_t elem) {   // every 8-pixel block row starts on 8 B (u8) / 16 B (f32)
    const size_t need = elem == 1 ? 8 : 16;
    return W % 8 == 0 && (uintptr_t)p % need == 0;
}

// in -> out for the pixels outside the first Hc rows x Wc columns (frames in chunks of gridDim.y)
void launch_copy_fringe(const uint8_t *in, uint8_t *out, int n, int H, int W, int Hc, int Wc, hipStream_t s) {
    const size_t fringe = (size_t)(H - Hc) * W * 3 + (size_t)Hc * (W - Wc) * 3;
    if (fringe == 0) return;
    const unsigned gx = (unsigned)((fringe + 256 * 4 - 1) / (256 * 4));
    for_chunks(n, kMaxChunk, [&](int f0, int cf) {
        const size_t fo = (size_t)f0 * H * W * 3;
        hipLaunchKernelGGL(copy_fringe_kernel, dim3(gx < 1024 ? gx : 1024, (unsigned)cf), dim3(256), 0, s, in + fo, out + fo, H, W, Hc, Wc);
        return OFMK_OK;
    });
}

// the same fringe into every copy of out ([copies][n][H][W][3])
int launch_copy_fringe_copies(const uint8_t *in, uint8_t *out, int copies, int n, int H, int W, hipStream_t s) {
    if (H % 8 == 0 && W % 8 == 0) return OFMK_OK;
    for (int q = 0; q < copies; ++q) launch_copy_fringe(in, out + (size_t)q * n * H * W * 3, n, H, W, (H / 8) * 8, (W / 8) * 8, s);
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// zero_counts (optional): [n][L] position sums of these frames, cleared by the kernel for a finalize that follows
int launch_analyze(const void *frames, int src, int n, int H, int W, const Workspace &ws, const Ctx &cx,
                   int32_t *zero_counts = nullptr, int L = 0) {
    hipStream_t s = cx.s;
    // (no fill dispatch in front: the frame mean is summed from per-tile partial sums that every launch writes in full -- common.hiph: emit_block)
    const Geom g = make_geom(H, W, ws, n);
    const dim3 grid = xcd_grid(g.nblk, n);
    ScopedTiming timing(KIND_ANALYZE, cx);
    // Occupancy cap by an (unused) dynamic LDS reservation: 48 KiB per workgroup = 3 workgroups per CU instead of the
    // 5 the registers allow.  Measured on the shipped kernel, interleaved in one session (profiles/r2_tuning_sweep.txt):
    // 3 per CU 0.341 ms, 4 or 5 per CU 0.350, 2 per CU 0.367, 1 per CU 0.553 -- fewer resident wavefronts keep the
    // window of frame bytes in flight smaller, which the memory system rewards (the bare read pattern shows the same).
    constexpr unsigned kAnalyzeLdsCap = 48u * 1024u;
    with_bool(aligned_rows(frames, W, src == SRC_RGB8 ? 1 : 4), [&](auto al) {
        constexpr bool AL = decltype(al)::value;
        if (src == SRC_RGB8) OFMK_TIMED_LAUNCH(timing, (analyze_kernel<SRC_RGB8, AL>), grid, dim3(kThreads), kAnalyzeLdsCap, s, frames, g, ws.rec, ws.ysum, zero_counts, L);
        else OFMK_TIMED_LAUNCH(timing, (analyze_kernel<SRC_YUV32F, AL>), grid, dim3(kThreads), 0, s, frames, g, ws.rec, ws.ysum, zero_counts, L);
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

int launch_finalize(FinArgs a, int n, const Ctx &cx) {
    const int per_wg = kThreads * kFinItems;
    const dim3 grid((unsigned)((a.N + per_wg - 1) / per_wg), (unsigned)n);
    ScopedTiming timing(KIND_FINALIZE, cx);
    with_bool(a.delta || a.soft || a.y_dc || a.lum || a.tex || a.step || a.c21_pre || a.c21_post, [&](auto full) {
        OFMK_TIMED_LAUNCH(timing, finalize_kernel<decltype(full)::value>, grid, dim3(kThreads), 0, cx.s, a);
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// What the DCT mark kernels (RGB, copies, planar) read besides the frames: the input frames' records in ws (launch_analyze).
MarkArgs mark_args(const Workspace &ws, int H, int W, const uint8_t *wm, int n_wm, const int32_t *wm_row, double alpha) {
    MarkArgs m;
    m.rec = ws.rec;
    m.ysum = ws.ysum;
    m.wm = wm;
    m.wm_row = wm_row;
    m.n_wm = n_wm;
    m.N = (int)((long long)H * W / 64);
    m.alpha = alpha;
    return m;
}

// Needs the input frames' records in ws.rec / ws.ysum (launch_analyze).  fused = true also leaves the
// MARKED frames' records in ws.rec and their partial sums in ws.ysum2.
int launch_mark_rgb8(const uint8_t *in, uint8_t *out, int n, int H, int W, const uint8_t *wm, int n_wm, const int32_t *wm_row,
                     double alpha, const Workspace &ws, bool fused, const Ctx &cx) {
    hipStream_t s = cx.s;
    const int xc = tile_xcds(cx, (size_t)n * H * W * 3);
    const Geom g = make_geom(H, W, ws, n, xc);
    const dim3 grid = xcd_grid(g.nblk, n, xc);
    const MarkArgs m = mark_args(ws, H, W, wm, n_wm, wm_row, alpha);
    {
        ScopedTiming timing(fused ? KIND_MARK_FUSED : KIND_MARK, cx);
        with_bool(aligned_rows(in, W, 1) && aligned_rows(out, W, 1), [&](auto al) {
            constexpr bool AL = decltype(al)::value;
            if (fused) OFMK_TIMED_LAUNCH(timing, (mark_rgb8_kernel<AL, true>), grid, dim3(kThreads), 0, s, in, out, g, m, ws.rec, ws.ysum2);
            // XCD-aware order: the marked rows are stored back to back at the end (dct_kernels.hiph: mark_rows HOLD; -2.5 %)
            else if (xc > 1) OFMK_TIMED_LAUNCH(timing, (mark_rgb8_kernel<AL, false, true>), grid, dim3(kThreads), 0, s, in, out, g, m, ws.rec, ws.ysum2);
            else OFMK_TIMED_LAUNCH(timing, (mark_rgb8_kernel<AL, false>), grid, dim3(kThreads), 0, s, in, out, g, m, ws.rec, ws.ysum2);
        });
    }
    HIP_TRY(hipGetLastError());
    if (in != out && (H % 8 || W % 8)) {
        launch_copy_fringe(in, out, n, H, W, (H / 8) * 8, (W / 8) * 8, s);
        HIP_TRY(hipGetLastError());
    }
    return OFMK_OK;
}

// The records a finalize launch works on: kRec planes of [frames][nblk] and the per-tile sums of those frames' block DCs.
struct RecView {
    const float *rec;
    const unsigned long long *ysum;    // [frames][tiles]
    size_t plane;                      // floats between the record planes
    int tiles;
};
RecView input_records(const Workspace &ws) { return {ws.rec, ws.ysum, ws.plane, ws.tiles}; }       // of the frames analyze saw
RecView marked_records(const Workspace &ws) { return {ws.rec, ws.ysum2, ws.plane, ws.tiles}; }     // of the frames a fused mark wrote

FinArgs fin_base(const RecView &v, int H, int W, double alpha) {
    FinArgs a;
    memset(&a, 0, sizeof(a));
    a.rec = v.rec;
    a.plane = v.plane;
    a.ysum = v.ysum;
    a.tiles = v.tiles;
    a.nblk = (H / 8) * (W / 8);
    a.N = (int)((long long)H * W / 64);
    a.L = 1;
    a.n_wm = 1;
    a.alpha = alpha;
    return a;
}

// float32 YUV plugin path, in place, after launch_analyze: separate scalar stage, then the rank-1 update of channel 1
int launch_mark_yuv32f(float *yuv, int n, int H, int W, const uint8_t *wm, int n_wm, const int32_t *wm_row, double alpha,
                       const Workspace &ws, const Ctx &cx) {
    FinArgs a = fin_base(input_records(ws), H, W, alpha);
    a.wm = wm;
    a.wm_row = wm_row;
    a.n_wm = n_wm;
    a.delta = ws.delta;
    if (int rc = launch_finalize(a, n, cx)) return rc;
    const Geom g = make_geom(H, W, ws);
    hipLaunchKernelGGL(mark_yuv32f_kernel, grid_2d(g.nblk, n), dim3(kThreads), 0, cx.s, yuv, g, ws.delta);
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

int launch_payloads(const int32_t *counts, int n, int L, int n_bits, const int32_t *perm, uint8_t *payload, hipStream_t s) {
    hipLaunchKernelGGL(degenerate_kernel, dim3((unsigned)n), dim3(kThreads), 0, s, counts, L, n_bits, perm, payload);
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// The copies half of a copies kernel's arguments, for a launch that starts at frame f0 of the call's n: wm_rows is the call's
// [copies][n] table or null, out the call's [copies][n] frames of frame_bytes.  Verify: a copy's counts are counts_per_frame
// int32 entries per frame (0 for the DCT codec's copies without a read-out), its bits bits_per_frame bytes.
CopyArgs make_copy_args(int copies, int n, int f0, const int32_t *wm_rows, size_t frame_bytes, size_t counts_per_frame = 0,
                        size_t bits_per_frame = 0) {
    CopyArgs k;
    memset(&k, 0, sizeof(k));
    k.copies = copies;
    k.rows_stride = n;
    k.wm_rows = wm_rows ? wm_rows + f0 : nullptr;
    k.out_stride = (size_t)n * frame_bytes;
    k.counts_stride = (size_t)n * counts_per_frame;
    k.bits_stride = (size_t)n * bits_per_frame;
    return k;
}

// One chunk of frames [f0, f0+cf) after launch_analyze left their records in ws: every copy of them in one launch.
int launch_mark_copies_rgb8(const uint8_t *in, uint8_t *out, int copies, int n, int f0, int cf, int H, int W, const uint8_t *wm,
                            int n_wm, const int32_t *wm_rows, double alpha, const Workspace &ws, const Ctx &cx) {
    const size_t fs = (size_t)H * W * 3;
    const uint8_t *pin = in + (size_t)f0 * fs;
    uint8_t *pout = out + (size_t)f0 * fs;
    const int xc = tile_xcds(cx, (size_t)cf * fs);
    const Geom g = make_geom(H, W, ws, cf, xc);
    const dim3 grid = xcd_grid(g.nblk, cf, xc);
    const MarkArgs m = mark_args(ws, H, W, wm, n_wm, nullptr, alpha);
    const CopyArgs k = make_copy_args(copies, n, f0, wm_rows, fs);
    ScopedTiming timing(KIND_MARK, cx);
    with_bool(aligned_rows(in, W, 1) && aligned_rows(out, W, 1), [&](auto al) {     // frame and copy strides are multiples of 8 when W is
        OFMK_TIMED_LAUNCH(timing, mark_copies_rgb8_kernel<decltype(al)::value>, grid, dim3(kThreads), 0, cx.s, pin, pout, g, m, k);
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// ---- the DCT codec's copies with verify (copies_kernels.hiph: mark_verify_copies_rgb8_kernel) ------------------------------
// The workspace of ofmk_embed_detect_copies_rgb8: the single-copy calls' arrays for the chunk's frames, and behind them every
// copy's own records and per-tile sums of the frames it was marked into.
struct CopiesWorkspace {
    Workspace base;               // the input frames' records (analyze); the separate route's detect of a copy reuses it
    float *rec;                   // kRec planes of [copies][frames][nblk]
    unsigned long long *ysum;     // [copies][frames][tiles]
    size_t plane;                 // copies * frames * nblk
};

size_t per_frame_copies_bytes(int copies, int H, int W) {
    const size_t nblk = (size_t)(H / 8) * (W / 8);
    return per_frame_bytes(H, W) + (size_t)copies * (nblk * kRec * sizeof(float) + tiles_per_frame(H, W) * 8);
}

int carve_copies(void *ws, size_t bytes, int copies, int H, int W, int want_frames, CopiesWorkspace &out) {
    if (!ws) return fail(OFMK_E_ARG, "workspace is null%s");
    if ((uintptr_t)ws % 256) return fail(OFMK_E_ARG, "workspace must be 256-byte aligned%s");
    const size_t per = per_frame_copies_bytes(copies, H, W);
    if (bytes < per + kFixedBytes) return fail(OFMK_E_WORKSPACE, "workspace smaller than ofmk_copies_workspace_bytes(1, copies, H, W)%s");
    size_t cap = (bytes - kFixedBytes) / per;
    if (want_frames > 0 && (size_t)want_frames < cap) cap = want_frames;
    if (cap > (size_t)kMaxChunk) cap = kMaxChunk;
    // the front of the buffer is the single-copy layout for `cap` frames (carve clamps to the same cap: it sees more bytes per frame)
    if (int rc = carve(ws, bytes, H, W, (int)cap, out.base)) return rc;
    const size_t nblk = (size_t)(H / 8) * (W / 8);
    char *p = reinterpret_cast<char *>(out.base.ysum2) + align256(cap * out.base.tiles * 8);
    out.plane = (size_t)copies * cap * nblk;
    out.rec = reinterpret_cast<float *>(p);
    p += align256(out.plane * kRec * sizeof(float));
    out.ysum = reinterpret_cast<unsigned long long *>(p);
    return OFMK_OK;
}

// copy q's records of the chunk's frames, left by a mark + verify copies launch
RecView copy_records(const CopiesWorkspace &ws, int q, int nblk) {
    return {ws.rec + (size_t)q * ws.base.frames * nblk, ws.ysum + (size_t)q * ws.base.frames * ws.base.tiles, ws.plane, ws.base.tiles};
}

// One chunk of frames [f0, f0+cf) after launch_analyze left their records in ws (the CopiesWorkspace's base): every copy of
// them, and every copy's records (v), in one launch.
int launch_mark_verify_copies_rgb8(const uint8_t *in, uint8_t *out, int copies, int n, int f0, int cf, int H, int W, const uint8_t *wm,
                                   int n_wm, const int32_t *wm_rows, double alpha, int L, const CopyRecs &v, const Workspace &ws,
                                   const Ctx &cx) {
    const size_t fs = (size_t)H * W * 3;
    const uint8_t *pin = in + (size_t)f0 * fs;
    uint8_t *pout = out + (size_t)f0 * fs;
    const int xc = tile_xcds(cx, (size_t)cf * fs);
    const Geom g = make_geom(H, W, ws, cf, xc);
    const dim3 grid = xcd_grid(g.nblk, cf, xc);
    const MarkArgs m = mark_args(ws, H, W, wm, n_wm, nullptr, alpha);
    const CopyArgs k = make_copy_args(copies, n, f0, wm_rows, fs, (size_t)L, (size_t)m.N);
    ScopedTiming timing(KIND_MARK_FUSED, cx);
    with_bool(aligned_rows(in, W, 1) && aligned_rows(out, W, 1), [&](auto al) {     // frame and copy strides are multiples of 8 when W is
        OFMK_TIMED_LAUNCH(timing, mark_verify_copies_rgb8_kernel<decltype(al)::value>, grid, dim3(kThreads), 0, cx.s, pin, pout, g, m, k, v);
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// ---- planar YUV 4:2:0 (I420 / NV12) -------------------------------------------------------------
int check_planar(int layout, int H, int W, const void *a, const void *b) {
    if (layout != OFMK_YUV_I420 && layout != OFMK_YUV_NV12) return fail(OFMK_E_ARG, "layout must be OFMK_YUV_I420 or OFMK_YUV_NV12%s");
    if (H % 8 || W % 8) return fail(OFMK_E_ARG, "planar 4:2:0 entry points need H and W to be multiples of 8%s");
    if ((a && (uintptr_t)a % 8) || (b && (uintptr_t)b % 8)) return fail(OFMK_E_ARG, "planar frame buffers must be 8-byte aligned%s");
    return OFMK_OK;
}

PGeom make_pgeom(int layout, int H, int W, size_t plane) {
    PGeom g;
    g.W = W;
    g.wb = W / 8;
    g.inv_wb = 1.0f / (float)g.wb;
    g.nblk = (H / 8) * (W / 8);
    g.frame_stride = (size_t)H * W * 3 / 2;
    g.u_off = (size_t)H * W;
    g.v_off = layout == OFMK_YUV_I420 ? g.u_off + (size_t)H * W / 4 : g.u_off + 1;
    g.cpitch = layout == OFMK_YUV_I420 ? W / 2 : W;
    g.plane = plane;
    return g;
}

int launch_analyze_yuv420(const uint8_t *frames, int layout, int n, int H, int W, const Workspace &ws, const Ctx &cx,
                          int32_t *zero_counts = nullptr, int L = 0) {
    const PGeom g = make_pgeom(layout, H, W, ws.plane);
    ScopedTiming timing(KIND_PLANAR_ANALYZE, cx);
    with_fmt(layout, [&](auto fmt) {
        OFMK_TIMED_LAUNCH(timing, analyze_yuv420_kernel<decltype(fmt)::value>, grid_2d(g.nblk, n), dim3(kThreads), 0, cx.s, frames, g, ws.rec, ws.ysum, zero_counts, L);
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

int launch_mark_yuv420(const uint8_t *in, uint8_t *out, int layout, int n, int H, int W, const uint8_t *wm, int n_wm, const int32_t *wm_row,
                       double alpha, const Workspace &ws, bool fused, const Ctx &cx) {
    const PGeom g = make_pgeom(layout, H, W, ws.plane);
    const MarkArgs m = mark_args(ws, H, W, wm, n_wm, wm_row, alpha);
    ScopedTiming timing(KIND_PLANAR_MARK, cx);
    with_fmt(layout, [&](auto fmt) { with_bool(fused, [&](auto fu) {
        OFMK_TIMED_LAUNCH(timing, (mark_yuv420_kernel<decltype(fmt)::value, decltype(fu)::value>), grid_2d(g.nblk, n), dim3(kThreads), 0, cx.s, in, out, g, m, ws.rec, ws.ysum2);
    }); });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// yuv [n] planar 4:2:0 frames <-> rgb [n][H][W][3], in the direction to_rgb says
int convert_yuv420(uint8_t *yuv, uint8_t *rgb, bool to_rgb, int layout, int n, int H, int W, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    int rc = check_dims(n, H, W);
    if (rc) return rc;
    if (!yuv || !rgb) return fail(OFMK_E_ARG, "null pointer%s");
    if ((rc = check_planar(layout, H, W, yuv, rgb))) return rc;
    const PGeom g = make_pgeom(layout, H, W, 0);
    hipStream_t s = static_cast<hipStream_t>(stream);
    for_chunks(n, kMaxChunk, [&](int f0, int cf) {
        uint8_t *py = yuv + (size_t)f0 * g.frame_stride, *pr = rgb + (size_t)f0 * H * W * 3;
        with_fmt(layout, [&](auto fmt) {
            if (to_rgb) hipLaunchKernelGGL(yuv420_to_rgb8_kernel<decltype(fmt)::value>, grid_2d(g.nblk, cf), dim3(kThreads), 0, s, py, pr, g);
            else hipLaunchKernelGGL(rgb8_to_yuv420_kernel<decltype(fmt)::value>, grid_2d(g.nblk, cf), dim3(kThreads), 0, s, pr, py, g);
        });
        return OFMK_OK;
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// ---- DwtDctSvd codec ---------------------------------------------------------------------------
// blk = 8: 16x16 pixel tiles (svd8_kernels.hiph).  a.N = H*W/64 (watermark row stride), a.N8 = H*W/256 (bits per frame).
Geom8 make_geom8(int H, int W) {
    Geom8 g;
    g.W = W;
    g.wt = ((W / 4) * 2) / 8;
    g.inv_wt = g.wt ? 1.0f / (float)g.wt : 0.f;
    g.ntile = (((H / 4) * 2) / 8) * g.wt;
    g.frames = 0;
    g.frame_stride = (size_t)H * W * 3;
    return g;
}

Geom svd_geom(int H, int W) {        // blk = 4: the DCT path's block geometry, no workspace behind it
    Workspace none;
    none.plane = 0;
    return make_geom(H, W, none);
}

// workgroups per frame of the DwtDctSvd frame kernels = rows of a frame's partial counts (OFMK_F_PARTIAL_COUNTS)
int svd_count_tiles(int H, int W, int blk) {
    const long long units = blk == 8 ? (long long)make_geom8(H, W).ntile : (long long)(H / 8) * (W / 8);
    return (int)((units + kThreads - 1) / kThreads);
}

// OFMK_F_PARTIAL_COUNTS on a DwtDctSvd read-out: the workgroup's sums live in its LDS histogram, so L is bounded by it
int check_partial(const ofmk_opts *o, int L, const int32_t *counts, int &partial) {
    partial = (o && (o->flags & OFMK_F_PARTIAL_COUNTS)) ? 1 : 0;
    if (partial && !counts) return fail(OFMK_E_ARG, "OFMK_F_PARTIAL_COUNTS without a counts buffer%s");
    if (partial && L > kHistMax) return fail(OFMK_E_ARG, "OFMK_F_PARTIAL_COUNTS needs L <= 2048 (longer payloads: plain counts)%s");
    return OFMK_OK;
}

int check_blk(int blk) {
    if (blk != 4 && blk != 8)
        return fail(OFMK_E_ARG, "blk must be 4 (the reference's default) or 8%s");
    return OFMK_OK;
}

// scales: host double[3], one per YUV channel (dwt_dct_svd_encoder.py:6: scales=[0,15,0]); <= 0 leaves a channel alone
int set_scales(SvdArgs &a, const double *scales, bool need_channel1) {
    if (!scales) return fail(OFMK_E_ARG, "scales is null (host array of 3 doubles)%s");
    bool any = false;
    for (int k = 0; k < 3; ++k) {
        if (!(scales[k] == scales[k]) || scales[k] > 1e30 || scales[k] < -1e30) return fail(OFMK_E_ARG, "scales must be finite%s");
        // decided on the float32 value the kernels use: a positive scale that is no normal float32 >= 1e-3 would mark
        // nothing (flushed to 0) or feed denormals to the quotient / remainder arithmetic
        const float sc = scales[k] > 0 ? (float)scales[k] : 0.f;
        if (scales[k] > 0 && !(sc >= 1.0e-3f)) return fail(OFMK_E_ARG, "a positive scale must be >= 1e-3 as float32%s");
        a.scales[k] = sc;
        any |= sc > 0.f;
    }
    if (!any && !need_channel1) return fail(OFMK_E_ARG, "no channel has a positive scale%s");
    return OFMK_OK;
}

// The kernel arguments of one DwtDctSvd call: scales, watermark (embed) and outputs (read-out; L is 1 without one).
// readout_opts: the call's opts where the call can read out -- OFMK_F_PARTIAL_COUNTS is then checked and taken; null for the
// embed-only calls, which ignore that flag.  need_channel1: a read-out alone accepts scales without a positive entry.
int make_svd_args(SvdArgs &a, int H, int W, const double *scales, bool need_channel1, const uint8_t *wm, int n_wm, const int32_t *wm_row,
                  int L, int32_t *counts, uint8_t *bits, const ofmk_opts *readout_opts) {
    memset(&a, 0, sizeof(a));
    if (int rc = set_scales(a, scales, need_channel1)) return rc;
    const bool readout = counts || bits;
    if (readout && L < 1) return fail(OFMK_E_ARG, "payload length L must be >= 1%s");     // the copies call's outputs are optional
    if (readout_opts)
        if (int rc = check_partial(readout_opts, L, counts, a.partial)) return rc;
    a.wm = wm;
    a.wm_row = wm_row;
    a.n_wm = n_wm;
    a.counts = counts;
    a.bits = bits;
    a.N = (int)((long long)H * W / 64);
    a.L = readout ? L : 1;
    return OFMK_OK;
}

// The kernels for 16x16 tiles take the same arguments plus N8 = H*W/256, the bits per frame (svd8_kernels.hiph).
Svd8Args to_args8(const SvdArgs &a, int N8) {
    Svd8Args b;
    memset(&b, 0, sizeof(b));
    b.wm = a.wm; b.wm_row = a.wm_row; b.n_wm = a.n_wm; b.counts = a.counts; b.bits = a.bits; b.partial = a.partial;
    b.N = a.N; b.N8 = N8; b.L = a.L;
    for (int k = 0; k < 3; ++k) b.scales[k] = a.scales[k];
    return b;
}

// scales[1] <= 0: the reference's decoder returns channel 1's (never written) bit array: all zeros
int zero_svd_readout(int n, int H, int W, int blk, const SvdArgs &a, hipStream_t s) {
    const size_t bits_per_frame = blk == 8 ? (size_t)((long long)H * W / 256) : (size_t)a.N;     // dwt_dct_svd_decoder.py:14
    if (a.counts) HIP_TRY(launch_zero(a.counts, (size_t)n * a.L * sizeof(int32_t) * (a.partial ? (size_t)svd_count_tiles(H, W, blk) : 1), s));
    if (a.bits) HIP_TRY(launch_zero(a.bits, (size_t)n * bits_per_frame, s));
    return OFMK_OK;
}

// The launch path of every DwtDctSvd frame kernel (RGB and planar 4:2:0, blk 4 and 8, A/B copies).  A variant says how much
// there is per frame; launch_svd clears the outputs, walks the frames in chunks of kMaxChunk and hands the variant one SvdChunk per
// launch.  All variants use the linear grid (one thread per unit, kThreads per workgroup), so partial counts have
// ofmk_svd_count_tiles(H, W, blk) rows.  The pixels the units do not cover are the variant's business after launch_svd returns.
struct SvdPlan {
    int units;              // threads per frame: (H/8)(W/8) blocks of 8x8 pixels (blk 4) or 16x16 tiles (blk 8)
    int bits_per_frame;     // N = H*W/64 (blk 4) or N8 = H*W/256 (blk 8); entries past `units` stay 0
    size_t frame_stride;    // bytes
    int copies;             // outputs per input frame: counts / bits are [copies][n][...]
    int count_words = 1;    // int32 words per entry of a.counts: 2 for the int64 soft sums of SVD_DETECT_SOFT (SvdArgs::counts)
};
struct SvdChunk {
    ScopedTiming timing;    // the KIND_SVD pair of this launch
    dim3 grid;
    size_t offset;          // bytes from the call's first frame to the chunk's
    int f0, frames;
    bool multi;             // a kernel that can mark channels 0 and 2 is needed
    SvdArgs a;              // wm_row / counts / bits start at the chunk's first frame
};

template <class Launch>
int launch_svd(const SvdPlan &p, int n, const SvdArgs &a, const Ctx &cx, Launch &&launch) {
    const size_t count_rows = a.partial ? (size_t)(p.units + kThreads - 1) / kThreads : 1;
    // partial counts: every workgroup stores its own row, nothing to clear (OFMK_F_PARTIAL_COUNTS); else the frames' [L] sums are added into
    if (a.counts && !a.partial) HIP_TRY(launch_zero(a.counts, (size_t)p.copies * n * a.L * sizeof(int32_t) * p.count_words, cx.s));
    if (a.bits && p.bits_per_frame > p.units) HIP_TRY(launch_zero(a.bits, (size_t)p.copies * n * p.bits_per_frame, cx.s));
    if (p.units == 0) return OFMK_OK;                // frames smaller than a 16x16 tile: no launch, no event pair
    const bool multi = a.scales[0] > 0.f || a.scales[2] > 0.f || !(a.scales[1] > 0.f);      // anything but the default [0, s, 0]
    for_chunks(n, kMaxChunk, [&](int f0, int cf) {
        SvdChunk c{ScopedTiming(KIND_SVD, cx), xcd_grid(p.units, cf), (size_t)f0 * p.frame_stride, f0, cf, multi, a};
        if (c.a.wm_row) c.a.wm_row += f0;
        if (c.a.counts) c.a.counts += (size_t)f0 * a.L * count_rows * p.count_words;
        if (c.a.bits) c.a.bits += (size_t)f0 * p.bits_per_frame;
        launch(c);
        return OFMK_OK;
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

int launch_svd_rgb8(const uint8_t *in, uint8_t *out, int n, int H, int W, int mode, int blk, const SvdArgs &a, const Ctx &cx) {
    int Hc = (H / 8) * 8, Wc = (W / 8) * 8;                // the region the units cover
    const bool reads = mode == SVD_DETECT || mode == SVD_DETECT_SOFT;      // no frames out
    const int cw = mode == SVD_DETECT_SOFT ? 2 : 1;
    int rc;
    if (blk == 8) {
        const Geom8 g = make_geom8(H, W);
        const int N8 = (int)((long long)H * W / 256);
        Hc = (((H / 4) * 2) / 8) * 16, Wc = g.wt * 16;
        const bool al = W % 8 == 0 && (uintptr_t)in % 8 == 0 && (reads || (uintptr_t)out % 8 == 0);
        rc = launch_svd({g.ntile, N8, g.frame_stride, 1, cw}, n, a, cx, [&](SvdChunk &c) {
            Geom8 gc = g;
            gc.frames = c.frames;
            with_bool(al, [&](auto al_) { with_svd_mode(mode, c.multi, [&](auto md, auto mu) {
                OFMK_TIMED_LAUNCH(c.timing, (svd8_rgb8_kernel<decltype(al_)::value, decltype(md)::value, decltype(mu)::value>), c.grid, dim3(kThreads), 0, cx.s,
                                  in + c.offset, out ? out + c.offset : nullptr, gc, to_args8(c.a, N8));
            }); });
        });
    } else {
        const Geom g = svd_geom(H, W);
        const bool al = aligned_rows(in, W, 1) && (reads || aligned_rows(out, W, 1));
        rc = launch_svd({g.nblk, a.N, g.frame_stride, 1, cw}, n, a, cx, [&](SvdChunk &c) {
            Geom gc = g;
            gc.frames = c.frames;
            with_bool(al, [&](auto al_) { with_svd_mode(mode, c.multi, [&](auto md, auto mu) {
                OFMK_TIMED_LAUNCH(c.timing, (svd_rgb8_kernel<decltype(al_)::value, decltype(md)::value, decltype(mu)::value>), c.grid, dim3(kThreads), 0, cx.s,
                                  in + c.offset, out ? out + c.offset : nullptr, gc, c.a);
            }); });
        });
    }
    if (rc) return rc;
    if (!reads && in != out && (Hc != H || Wc != W)) {
        launch_copy_fringe(in, out, n, H, W, Hc, Wc, cx.s);
        HIP_TRY(hipGetLastError());
    }
    return OFMK_OK;
}

// Planar YUV 4:2:0 (svd_planar_kernels.hiph).  blk = 4: the 8x8 blocks cover the frame (H and W are multiples of 8).  blk = 8: the
// pixels outside the tiles' Hc x Wc region come out as the chain's: the 4:2:0 round trip of the input, written by one more
// launch (also timed under KIND_SVD) -- also in place, where the RGB path has nothing to copy.
int launch_svd_yuv420(const uint8_t *in, uint8_t *out, int layout, int n, int H, int W, int mode, int blk, const SvdArgs &a, const Ctx &cx) {
    const PGeom g = make_pgeom(layout, H, W, 0);
    const int cw = mode == SVD_DETECT_SOFT ? 2 : 1;
    if (blk == 4)
        return launch_svd({g.nblk, a.N, g.frame_stride, 1, cw}, n, a, cx, [&](SvdChunk &c) {
            with_fmt(layout, [&](auto fmt) { with_svd_mode(mode, c.multi, [&](auto md, auto mu) {
                OFMK_TIMED_LAUNCH(c.timing, (svd_yuv420_kernel<decltype(fmt)::value, decltype(md)::value, decltype(mu)::value>), c.grid, dim3(kThreads), 0, cx.s,
                                  in + c.offset, out ? out + c.offset : nullptr, g, c.frames, c.a);
            }); });
        });
    const Geom8 g8 = make_geom8(H, W);
    const int N8 = (int)((long long)H * W / 256);
    int rc = launch_svd({g8.ntile, N8, g.frame_stride, 1, cw}, n, a, cx, [&](SvdChunk &c) {
        Geom8 gc = g8;
        gc.frames = c.frames;
        with_fmt(layout, [&](auto fmt) { with_svd_mode(mode, c.multi, [&](auto md, auto mu) {
            OFMK_TIMED_LAUNCH(c.timing, (svd8_yuv420_kernel<decltype(fmt)::value, decltype(md)::value, decltype(mu)::value>), c.grid, dim3(kThreads), 0, cx.s,
                              in + c.offset, out ? out + c.offset : nullptr, g, gc, to_args8(c.a, N8));
        }); });
    });
    if (rc) return rc;
    const int hcb = (((H / 4) * 2) / 8) * 2, wcb = g8.wt * 2;                 // the tiles' Hc x Wc region in 8x8 pixel blocks
    const int nfringe = g.nblk - hcb * wcb;
    if (mode == SVD_DETECT || mode == SVD_DETECT_SOFT || nfringe <= 0) return OFMK_OK;
    for_chunks(n, kMaxChunk, [&](int f0, int cf) {
        const size_t fo = (size_t)f0 * g.frame_stride;
        ScopedTiming timing(KIND_SVD, cx);
        with_fmt(layout, [&](auto fmt) {
            OFMK_TIMED_LAUNCH(timing, svd_fringe_yuv420_kernel<decltype(fmt)::value>, grid_2d(nfringe, cf), dim3(kThreads), 0, cx.s, in + fo, out + fo, g, hcb, wcb, nfringe);
        });
        return OFMK_OK;
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// The DwtDctSvd soft read-out behind ofmk_svd_detect_soft_*: the int64 [n][L] sums travel in SvdArgs::counts; OFMK_F_PARTIAL_COUNTS
// is not looked at (the soft sums have no partial form); scales[1] <= 0: all zeros, as the hard read-out.  launch(a) is the
// variant's launcher in SVD_DETECT_SOFT mode.
template <class Launch>
int svd_detect_soft(int n, int H, int W, int L, const double *scales, long long *soft, void *stream, Launch &&launch) {
    SvdArgs a;
    if (int rc = make_svd_args(a, H, W, scales, true, nullptr, 0, nullptr, L, reinterpret_cast<int32_t *>(soft), nullptr, nullptr)) return rc;
    if (a.scales[1] > 0.f) return launch(a);
    HIP_TRY(launch_zero(soft, (size_t)n * L * sizeof(long long), static_cast<hipStream_t>(stream)));
    return OFMK_OK;
}

// ---- block-grid resync of cropped and rescaled frames, DwtDctSvd (blk 4, channel 1) ------------------------------------------------
// The checks the DwtDctSvd resync and warp calls share on top of their own: blk 4 only, finite scales, and -- need_mark -- a marked
// channel 1.
int check_resync_scales(SvdArgs &a, const double *scales, int blk, bool need_mark) {
    if (blk != 4) return fail(OFMK_E_ARG, "the resync calls are for blk 4%s");
    memset(&a, 0, sizeof(a));
    if (int rc = set_scales(a, scales, true)) return rc;
    if (need_mark && !(a.scales[1] > 0.f)) return fail(OFMK_E_ARG, "scales[1] must be positive: the phase search reads channel 1%s");
    return OFMK_OK;
}

// ---- rescaled leaks (warp_kernels.hiph) -----------------------------------------------------------------------------------------
static_assert(sizeof(WarpMap) == sizeof(ofmk_warp) && sizeof(ofmk_warp) == 32, "ofmk_warp is four int64");

// a leak may be smaller than one unit: upscaled it can still fill canvas units
int check_leak_dims(int h, int w) {
    if (h < 1 || w < 1 || (long long)h * w >= (1LL << 28)) return fail(OFMK_E_ARG, "leak h, w must be positive with h*w < 2^28%s");
    return OFMK_OK;
}

int check_map(const ofmk_warp *geom, WarpMap &m) {
    m.ay = geom->ay; m.by = geom->by; m.ax = geom->ax; m.bx = geom->bx;
    if (!warp_map_ok(m)) return fail(OFMK_E_ARG, "ofmk_warp: ay, ax must be in [2^12, 2^20] and |by|, |bx| <= 2^48%s");
    return OFMK_OK;
}

// Units [u0, u1) of one axis whose 8 pixels are inside a leak of `len` samples.  Both conditions are monotone in u (a > 0): the
// first pixel's pos >= 0 holds from some unit on, the last pixel's sample <= len - 1 up to some unit.
void warp_axis_units(long long a, long long b, int len, int units, int &u0, int &u1) {
    int lo = 0, hi = units;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (a * (8LL * mid) + b >= 0) hi = mid; else lo = mid + 1;
    }
    u0 = lo;
    lo = 0; hi = units;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (((a * (8LL * mid + 7) + b) >> 16) > (long long)(len - 1)) hi = mid; else lo = mid + 1;
    }
    u1 = lo;
}

void units_rect(const WarpMap &m, int h, int w, int H, int W, int out[4]) {
    int i0, i1, j0, j1;
    warp_axis_units(m.ay, m.by, h, H / 8, i0, i1);
    warp_axis_units(m.ax, m.bx, w, W / 8, j0, j1);
    const bool any = i0 < i1 && j0 < j1;
    out[0] = any ? i0 : 0; out[1] = any ? i1 : 0; out[2] = any ? j0 : 0; out[3] = any ? j1 : 0;
}

// ---- rotated leaks (affine_kernels.hiph) ---------------------------------------------------------------------------------------
static_assert(sizeof(AffineMap) == sizeof(ofmk_affine) && sizeof(ofmk_affine) == 48, "ofmk_affine is six int64");

int check_map(const ofmk_affine *geom, AffineMap &m) {
    m.ayy = geom->ayy; m.ayx = geom->ayx; m.by = geom->by; m.axy = geom->axy; m.axx = geom->axx; m.bx = geom->bx;
    if (!affine_map_ok(m))
        return fail(OFMK_E_ARG, "ofmk_affine: coefficients must be in [-2^20, 2^20], |by|, |bx| <= 2^48 and |ayy*axx - ayx*axy| >= 2^24%s");
    return OFMK_OK;
}

// The integers j with a * j + c >= 0, cut out of [lo, hi].
void affine_bound(long long a, long long c, long long &lo, long long &hi) {
    if (a == 0) {
        if (c < 0) hi = -1;                                     // lo >= 0 throughout: empty
        return;
    }
    const long long d = a > 0 ? a : -a, n = a > 0 ? -c + a - 1 : c;      // a > 0: j >= ceil(-c / a); a < 0: j <= floor(c / -a)
    long long q = n / d;
    if (n % d < 0) --q;
    if (a > 0) lo = q > lo ? q : lo;
    else hi = q < hi ? q : hi;
}

// out = {i0, i1, j0, j1, count}: the bounding rectangle of the counting units and how many count; all 0 when none does.  Each of a
// unit's 16 conditions (4 corner pixels x 4 edges of the leak) is linear in j, so a row of units counts on an interval of j.
void units_rect(const AffineMap &m, int h, int w, int H, int W, int out[5]) {
    const int rows = H / 8, cols = W / 8;
    int i0 = rows, i1 = 0, j0 = cols, j1 = 0, count = 0;
    for (int i = 0; i < rows; ++i) {
        long long lo = 0, hi = cols - 1;
        for (int corner = 0; corner < 4; ++corner) {
            const int y = 8 * i + (corner & 2 ? 7 : 0), dx = corner & 1 ? 7 : 0;
            const long long cy = affine_pos_y(m, y, dx), cx = affine_pos_x(m, y, dx);      // pixel (y, 8 j + dx): cy + 8 ayx j, cx + 8 axx j
            affine_bound(8 * m.ayx, cy, lo, hi);
            affine_bound(-8 * m.ayx, ((long long)h << 16) - 1 - cy, lo, hi);
            affine_bound(8 * m.axx, cx, lo, hi);
            affine_bound(-8 * m.axx, ((long long)w << 16) - 1 - cx, lo, hi);
        }
        if (lo > hi) continue;
        i0 = i < i0 ? i : i0; i1 = i + 1;
        j0 = (int)lo < j0 ? (int)lo : j0; j1 = (int)hi + 1 > j1 ? (int)hi + 1 : j1;
        count += (int)(hi - lo + 1);
    }
    out[0] = count ? i0 : 0; out[1] = i1; out[2] = count ? j0 : 0; out[3] = j1; out[4] = count;
}

// ---- what the leak-geometry calls share, under either map (WarpMap with ofmk_warp, AffineMap with ofmk_affine) ---------------------
int check_canvas(int H, int W) {
    if (H < 1 || W < 1 || (long long)H * W >= (1LL << 28)) return fail(OFMK_E_ARG, "canvas H, W must be positive with H*W < 2^28%s");
    return OFMK_OK;
}

int check_out_rect(int Hout, int Wout, int oy, int ox) {
    if (Hout < 1 || Wout < 1 || (long long)Hout * Wout >= (1LL << 28)) return fail(OFMK_E_ARG, "Hout, Wout must be positive with Hout*Wout < 2^28%s");
    if (oy < 0 || ox < 0 || oy >= (1 << 28) || ox >= (1 << 28)) return fail(OFMK_E_ARG, "oy, ox must be in [0, 2^28)%s");
    return OFMK_OK;
}

// The checks of the calls that take a candidate list: ptrs = "every pointer is non-null"; max_side > 0 bounds the canvas sides, `why` ends its message.
int check_search_args(const ofmk_opts *opts, int n, int h, int w, int H, int W, bool ptrs, int K, int max_side = 0, const char *why = "") {
    if (int orc = check_opts(opts)) return orc;
    if (int rc = check_dims(n, H, W)) return rc;
    if (max_side > 0 && (H > max_side || W > max_side)) return fail(OFMK_E_ARG, "canvas H, W must be at most 4096%s", why);
    if (int rc = check_leak_dims(h, w)) return rc;
    if (!ptrs) return fail(OFMK_E_ARG, "null pointer%s");
    if (K < 1) return fail(OFMK_E_ARG, "K must be at least 1%s");
    if ((long long)n * K >= (1LL << 40)) return fail(OFMK_E_ARG, "n * K must be < 2^40%s");
    return OFMK_OK;
}

// Candidates [0, K) in gridDim.y and frames [0, n) in gridDim.z, both in chunks of at most kMaxChunk, with units_per_pair workgroups
// per frame and candidate in gridDim.x: body(k0, ck, f0, cf), until one returns an error code.
template <class Body>
int for_cand_frame_chunks(long long units_per_pair, int K, int n, Body &&body) {
    return for_chunks(K, kMaxChunk, [&](int k0, int ck) {
        const long long room = (1LL << 30) / (units_per_pair * ck);              // workgroups per launch stay below 2^30
        const int cap = room < 1 ? 1 : room > kMaxChunk ? kMaxChunk : (int)room;
        return for_chunks(n, cap, [&](int f0, int cf) { return body(k0, ck, f0, cf); });
    });
}

// out = the counting rectangle of canvas units under *geom (units_rect): ofmk_warp_units / ofmk_affine_units.
template <class Map, class Geom>
int map_units(int h, int w, int H, int W, const Geom *geom, int *out) {
    if (!geom || !out) return fail(OFMK_E_ARG, "null pointer%s");
    if (int rc = check_leak_dims(h, w)) return rc;
    if (int rc = check_canvas(H, W)) return rc;
    Map m;
    if (int rc = check_map(geom, m)) return rc;
    units_rect(m, h, w, H, W, out);
    return OFMK_OK;
}

// The leak resampled onto a canvas rectangle: ofmk_warp_rgb8 (Args = WarpArgs; takes no timing pair) / ofmk_warp_affine_rgb8.
template <class Args, auto Kernel, bool kTimed, class Geom>
int warp_frames(const uint8_t *in, int n, int h, int w, uint8_t *out, int Hout, int Wout, int oy, int ox, const Geom *geom, void *stream,
                const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    if (n <= 0) return fail(OFMK_E_ARG, "n must be positive%s");
    if (!in || !out || !geom) return fail(OFMK_E_ARG, "null pointer%s");
    if (int rc = check_leak_dims(h, w)) return rc;
    if (int rc = check_out_rect(Hout, Wout, oy, ox)) return rc;
    Args a;
    if (int rc = check_map(geom, a.m)) return rc;
    Ctx cx = make_ctx(stream, opts);
    if (!kTimed) cx.t = nullptr;
    a.h = h; a.w = w; a.Hout = Hout; a.Wout = Wout; a.oy = oy; a.ox = ox;
    a.in_stride = (size_t)h * w * 3;
    a.out_stride = (size_t)Hout * Wout * 3;
    for_chunks(n, kMaxChunk, [&](int f0, int cf) {
        ScopedTiming timing(KIND_SVD, cx);
        OFMK_TIMED_LAUNCH(timing, Kernel, grid_2d(Hout * Wout, cf), dim3(kThreads), 0, cx.s, in + (size_t)f0 * a.in_stride,
                          out + (size_t)f0 * a.out_stride, a);
        return OFMK_OK;
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// The soft read-out of the counting units of the leak under *geom: ofmk_svd_detect_soft_warp_rgb8 / ofmk_svd_detect_soft_affine_rgb8.
template <class Args, auto Kernel, class Geom>
int svd_detect_soft_mapped(const uint8_t *in, int n, int h, int w, int H, int W, const Geom *geom, int L, const double *scales, int blk,
                           long long *soft, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    if (int rc = check_soft_args(in, n, H, W, L, soft)) return rc;
    if (int rc = check_leak_dims(h, w)) return rc;
    if (!geom) return fail(OFMK_E_ARG, "null pointer%s");
    Args a;
    if (int rc = check_map(geom, a.m)) return rc;
    SvdArgs sa;
    if (int rc = check_resync_scales(sa, scales, blk, false)) return rc;
    const Ctx cx = make_ctx(stream, opts);
    HIP_TRY(launch_zero(soft, (size_t)n * L * sizeof(long long), cx.s));
    int r[5];
    units_rect(a.m, h, w, H, W, r);
    if (!(sa.scales[1] > 0.f) || r[1] == r[0]) return OFMK_OK;                   // no unit counts: both rectangles are then all 0
    a.h = h; a.w = w;
    a.i0 = r[0]; a.j0 = r[2];
    a.cols = r[3] - r[2];
    a.nunits = (r[1] - r[0]) * a.cols;
    a.canvas_cols = W / 8;
    a.L = L;
    a.frame_stride = (size_t)h * w * 3;
    a.scale = sa.scales[1];
    for_chunks(n, kMaxChunk, [&](int f0, int cf) {
        ScopedTiming timing(KIND_SVD, cx);
        Args ac = a;
        ac.frames = cf;
        ac.soft = soft + (size_t)f0 * L;
        OFMK_TIMED_LAUNCH(timing, Kernel, xcd_grid(a.nunits, cf), dim3(kThreads), 0, cx.s, in + (size_t)f0 * a.frame_stride, ac);
        return OFMK_OK;
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// ---- C marked copies of the same frames (copies_kernels.hiph) -------------------------------------------------------
constexpr int kMaxCopies = 16;       // a payload's copy field has 4 bits (fingerprint.payload_for_segment)

// blk = 8 has no fused copies kernel for its 16x16 tiles: the single-copy launches once per copy.  launch(out_q, a_q) is that
// launcher on copy q's frames, with copy q's watermark rows, counts and bits.
template <class Launch>
int launch_svd8_copies(uint8_t *out, size_t frame_bytes, int copies, int n, int H, int W, const int32_t *wm_rows, const SvdArgs &a,
                       Launch &&launch) {
    const size_t count_rows = a.partial ? (size_t)svd_count_tiles(H, W, 8) : 1;
    const size_t bits8 = (size_t)((long long)H * W / 256);
    for (int q = 0; q < copies; ++q) {
        SvdArgs b = a;
        if (wm_rows) {
            b.wm_row = wm_rows + (size_t)q * n;
        } else {                                      // row q (clamped) for every frame: that row as a one-row table
            b.wm = a.wm + (size_t)(q < a.n_wm - 1 ? q : a.n_wm - 1) * a.N;
            b.n_wm = 1;
        }
        if (b.counts) b.counts += (size_t)q * n * a.L * count_rows;
        if (b.bits) b.bits += (size_t)q * n * bits8;
        if (int rc = launch(out + (size_t)q * n * frame_bytes, b)) return rc;
    }
    return OFMK_OK;
}

// The argument checks every copies call shares: copies in range, out ([copies][n] frames of frame_bytes: H*W*3 as RGB, H*W*3/2
// as 4:2:0 planes) not overlapping in ([n] frames).
int check_copies(const void *in, const void *out, int copies, int n, size_t frame_bytes) {
    if (copies < 1 || copies > kMaxCopies) return fail(OFMK_E_ARG, "copies must be in [1, 16]%s");
    const size_t fb = (size_t)n * frame_bytes;
    const uintptr_t i0 = (uintptr_t)in, o0 = (uintptr_t)out;
    if (o0 < i0 + fb && i0 < o0 + fb * (size_t)copies) return fail(OFMK_E_ARG, "out must not overlap in (no in-place copies)%s");
    return OFMK_OK;
}

// blk = 4: every copy from one launch per kMaxChunk frames; counts / bits of copy q at q * (the single-copy call's size).
// a.wm_row is null: the rows come from wm_rows ([copies][n], or null = copy q marks with row q).
// soft (optional): the call's int64 [copies][n][L] soft sums, cleared by the caller; a.L is then the payload length whether or not
// counts / bits are asked for (svd_copies_soft_rgb8_kernel).
int launch_svd_copies_rgb8(const uint8_t *in, uint8_t *out, int copies, int n, int H, int W, const int32_t *wm_rows, const SvdArgs &a,
                           const Ctx &cx, long long *soft = nullptr) {
    const Geom g = svd_geom(H, W);
    const bool verify = a.counts || a.bits;
    const size_t count_rows = a.partial ? (size_t)svd_count_tiles(H, W, 4) : 1;
    const bool al = aligned_rows(in, W, 1) && aligned_rows(out, W, 1);
    int rc = launch_svd({g.nblk, a.N, g.frame_stride, copies}, n, a, cx, [&](SvdChunk &c) {
        const CopyArgs kc = make_copy_args(copies, n, c.f0, wm_rows, g.frame_stride, count_rows * a.L, a.N);
        Geom gc = g;
        gc.frames = c.frames;
        if (soft) {
            const CopySoft sf{soft + (size_t)c.f0 * a.L, (size_t)n * a.L};
            with_bool(al, [&](auto al_) { with_bool(c.multi, [&](auto mu) {
                OFMK_TIMED_LAUNCH(c.timing, (svd_copies_soft_rgb8_kernel<decltype(al_)::value, decltype(mu)::value>), c.grid, dim3(kThreads), 0, cx.s,
                                  in + c.offset, out + c.offset, gc, c.a, kc, sf);
            }); });
            return;
        }
        with_bool(al, [&](auto al_) { with_bool(verify, [&](auto vf) { with_bool(c.multi, [&](auto mu) {
            OFMK_TIMED_LAUNCH(c.timing, (svd_copies_rgb8_kernel<decltype(al_)::value, decltype(vf)::value, decltype(mu)::value>), c.grid, dim3(kThreads), 0, cx.s,
                              in + c.offset, out + c.offset, gc, c.a, kc);
        }); }); });
    });
    if (rc) return rc;
    return launch_copy_fringe_copies(in, out, copies, n, H, W, cx.s);
}

// The same on 4:2:0 planes (planar_copies_kernels.hiph).  One chunk of frames [f0, f0+cf) after launch_analyze_yuv420 left their
// records in ws: every copy of them in one launch.
int launch_mark_copies_yuv420(const uint8_t *in, uint8_t *out, int layout, int copies, int n, int f0, int cf, int H, int W,
                              const uint8_t *wm, int n_wm, const int32_t *wm_rows, double alpha, const Workspace &ws, const Ctx &cx) {
    const PGeom g = make_pgeom(layout, H, W, ws.plane);
    const MarkArgs m = mark_args(ws, H, W, wm, n_wm, nullptr, alpha);
    const CopyArgs k = make_copy_args(copies, n, f0, wm_rows, g.frame_stride);
    const size_t fo = (size_t)f0 * g.frame_stride;
    ScopedTiming timing(KIND_PLANAR_MARK, cx);
    with_fmt(layout, [&](auto fmt) {
        OFMK_TIMED_LAUNCH(timing, mark_copies_yuv420_kernel<decltype(fmt)::value>, grid_2d(g.nblk, cf), dim3(kThreads), 0, cx.s, in + fo, out + fo, g, m, k);
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// launch_mark_verify_copies_rgb8 on planes (planar_copies_kernels.hiph: mark_verify_copies_yuv420_kernel): every copy of frames
// [f0, f0+cf) and every copy's records (v) in one launch, after launch_analyze_yuv420 left the input's records in ws.  The grid
// is grid_2d's: its x extent is the tile count emit_block files the per-tile sums under, and it is ws.tiles (both are
// ceil(nblk / kThreads)), which is what fin_base hands finalize.
int launch_mark_verify_copies_yuv420(const uint8_t *in, uint8_t *out, int layout, int copies, int n, int f0, int cf, int H, int W,
                                     const uint8_t *wm, int n_wm, const int32_t *wm_rows, double alpha, int L, const CopyRecs &v,
                                     const Workspace &ws, const Ctx &cx) {
    const PGeom g = make_pgeom(layout, H, W, ws.plane);
    const MarkArgs m = mark_args(ws, H, W, wm, n_wm, nullptr, alpha);
    const CopyArgs k = make_copy_args(copies, n, f0, wm_rows, g.frame_stride, (size_t)L, (size_t)m.N);
    const dim3 grid = grid_2d(g.nblk, cf);
    if ((int)grid.x != ws.tiles) return fail(OFMK_E_ARG, "internal: tile count of the launch and of the workspace differ%s");
    const size_t fo = (size_t)f0 * g.frame_stride;
    ScopedTiming timing(KIND_PLANAR_MARK, cx);
    with_fmt(layout, [&](auto fmt) {
        OFMK_TIMED_LAUNCH(timing, mark_verify_copies_yuv420_kernel<decltype(fmt)::value>, grid, dim3(kThreads), 0, cx.s, in + fo, out + fo, g, m, k, v);
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// blk = 4 on planes: every copy from one launch per kMaxChunk frames, as launch_svd_copies_rgb8 (H and W multiples of 8: no fringe).
// soft: as launch_svd_copies_rgb8 (svd_copies_soft_yuv420_kernel).
int launch_svd_copies_yuv420(const uint8_t *in, uint8_t *out, int layout, int copies, int n, int H, int W, const int32_t *wm_rows,
                             const SvdArgs &a, const Ctx &cx, long long *soft = nullptr) {
    const PGeom g = make_pgeom(layout, H, W, 0);
    const bool verify = a.counts || a.bits;
    const size_t count_rows = a.partial ? (size_t)svd_count_tiles(H, W, 4) : 1;
    return launch_svd({g.nblk, a.N, g.frame_stride, copies}, n, a, cx, [&](SvdChunk &c) {
        const CopyArgs kc = make_copy_args(copies, n, c.f0, wm_rows, g.frame_stride, count_rows * a.L, a.N);
        if (soft) {
            const CopySoft sf{soft + (size_t)c.f0 * a.L, (size_t)n * a.L};
            with_fmt(layout, [&](auto fmt) { with_bool(c.multi, [&](auto mu) {
                OFMK_TIMED_LAUNCH(c.timing, (svd_copies_soft_yuv420_kernel<decltype(fmt)::value, decltype(mu)::value>), c.grid, dim3(kThreads), 0, cx.s,
                                  in + c.offset, out + c.offset, g, c.frames, c.a, kc, sf);
            }); });
            return;
        }
        with_fmt(layout, [&](auto fmt) { with_bool(verify, [&](auto vf) { with_bool(c.multi, [&](auto mu) {
            OFMK_TIMED_LAUNCH(c.timing, (svd_copies_yuv420_kernel<decltype(fmt)::value, decltype(vf)::value, decltype(mu)::value>), c.grid, dim3(kThreads), 0, cx.s,
                              in + c.offset, out + c.offset, g, c.frames, c.a, kc);
        }); }); });
    });
}

// The host half of ofmk_svd_embed_copies_soft_*: the hard copies call plus the int64 [copies][n][L] soft sums of every written copy.
// Arguments are checked by the caller; a is the hard call's SvdArgs.  scales[1] <= 0: the hard call's route, soft stays zero.
// blk 4: fused(a, soft) is the copies launcher (soft null: its hard form); blk 8: single(out_q, b) is the single-copy embed (+ verify)
// launcher on copy q, and soft_of(out_q, b) the stand-alone soft read-out of that written copy (b.counts carries the int64 sums).
template <class Fused, class Single, class SoftOf>
int svd_copies_soft(uint8_t *out, size_t frame_bytes, int copies, int n, int H, int W, int blk, int L, const int32_t *wm_rows, SvdArgs a,
                    long long *soft, const Ctx &cx, Fused &&fused, Single &&single, SoftOf &&soft_of) {
    a.L = L;                                           // also without counts / bits: the soft sums' row length
    HIP_TRY(launch_zero(soft, (size_t)copies * n * L * sizeof(long long), cx.s));
    const bool on = a.scales[1] > 0.f;
    if (blk == 4) return fused(a, on ? soft : nullptr);
    return launch_svd8_copies(out, frame_bytes, copies, n, H, W, wm_rows, a, [&](uint8_t *out_q, const SvdArgs &b) {
        if (int rc = single(out_q, b)) return rc;
        if (!on) return (int)OFMK_OK;
        const size_t q = (size_t)(out_q - out) / ((size_t)n * frame_bytes);
        SvdArgs bs = b;
        bs.counts = reinterpret_cast<int32_t *>(soft + q * n * L);
        bs.bits = nullptr;
        bs.partial = 0;
        return soft_of(out_q, bs);
    });
}

// ---- the DCT codec's call path: one for every frame format -------------------------------------------------------------------
// What the frames of a call are.  An entry point makes it once, after the checks its format needs; the four leaf launchers
// below (analyze_frames, mark_frames, mark_copies, mark_verify_copies) pick the format's own launcher, and nothing else asks:
// everything past them works on frames of frame_bytes bytes and on the records in the workspace, which are the same for all.
enum FrameKind { FRAMES_RGB8, FRAMES_YUV32F, FRAMES_YUV420 };
struct FrameFmt {
    FrameKind kind;
    int layout;            // FRAMES_YUV420: OFMK_YUV_I420 / OFMK_YUV_NV12
    int H, W;
    size_t frame_bytes;
};
FrameFmt rgb8_frames(int H, int W) { return {FRAMES_RGB8, 0, H, W, (size_t)H * W * 3}; }
FrameFmt yuv32f_frames(int H, int W) { return {FRAMES_YUV32F, 0, H, W, (size_t)H * W * 3 * sizeof(float)}; }
FrameFmt yuv420_frames(int layout, int H, int W) { return {FRAMES_YUV420, layout, H, W, (size_t)H * W * 3 / 2}; }

// n frames' records into ws; zero_counts: as launch_analyze
int analyze_frames(const FrameFmt &f, const uint8_t *frames, int n, const Workspace &ws, const Ctx &cx, int32_t *zero_counts = nullptr,
                   int L = 0) {
    if (f.kind == FRAMES_YUV420) return launch_analyze_yuv420(frames, f.layout, n, f.H, f.W, ws, cx, zero_counts, L);
    return launch_analyze(frames, f.kind == FRAMES_RGB8 ? SRC_RGB8 : SRC_YUV32F, n, f.H, f.W, ws, cx, zero_counts, L);
}

// Needs the input frames' records in ws (analyze_frames).  fused = true also leaves the MARKED frames' records there
// (marked_records); the float32 frames of the plugin path have no fused kernel and are marked in place.
int mark_frames(const FrameFmt &f, const uint8_t *in, uint8_t *out, int n, const uint8_t *wm, int n_wm, const int32_t *wm_row,
                double alpha, const Workspace &ws, bool fused, const Ctx &cx) {
    if (f.kind == FRAMES_RGB8) return launch_mark_rgb8(in, out, n, f.H, f.W, wm, n_wm, wm_row, alpha, ws, fused, cx);
    if (f.kind == FRAMES_YUV420) return launch_mark_yuv420(in, out, f.layout, n, f.H, f.W, wm, n_wm, wm_row, alpha, ws, fused, cx);
    if (fused || in != out) return fail(OFMK_E_ARG, "internal: float32 frames are marked in place, without verify%s");
    return launch_mark_yuv32f(reinterpret_cast<float *>(out), n, f.H, f.W, wm, n_wm, wm_row, alpha, ws, cx);
}

// Every copy of frames [f0, f0+cf) of the call's n in one launch, after analyze_frames left their records in ws.
int mark_copies(const FrameFmt &f, const uint8_t *in, uint8_t *out, int copies, int n, int f0, int cf, const uint8_t *wm, int n_wm,
                const int32_t *wm_rows, double alpha, const Workspace &ws, const Ctx &cx) {
    if (f.kind == FRAMES_RGB8) return launch_mark_copies_rgb8(in, out, copies, n, f0, cf, f.H, f.W, wm, n_wm, wm_rows, alpha, ws, cx);
    if (f.kind == FRAMES_YUV420)
        return launch_mark_copies_yuv420(in, out, f.layout, copies, n, f0, cf, f.H, f.W, wm, n_wm, wm_rows, alpha, ws, cx);
    return fail(OFMK_E_ARG, "internal: no copies kernel for float32 frames%s");
}

// The same, and every copy's own records (copy_records) in that launch; zero_counts (the call's [copies][n][L] counts, or null)
// is cleared for these frames in every copy.
int mark_verify_copies(const FrameFmt &f, const uint8_t *in, uint8_t *out, int copies, int n, int f0, int cf, const uint8_t *wm,
                       int n_wm, const int32_t *wm_rows, double alpha, int L, int32_t *zero_counts, const CopiesWorkspace &ws,
                       const Ctx &cx) {
    CopyRecs v;
    v.rec = ws.rec;
    v.ysum = ws.ysum;
    v.plane = ws.plane;
    v.rec_stride = (size_t)ws.base.frames * (f.H / 8) * (f.W / 8);
    v.ysum_stride = (size_t)ws.base.frames * ws.base.tiles;
    v.zero_counts = zero_counts ? zero_counts + (size_t)f0 * L : nullptr;
    v.L = L;
    if (f.kind == FRAMES_RGB8)
        return launch_mark_verify_copies_rgb8(in, out, copies, n, f0, cf, f.H, f.W, wm, n_wm, wm_rows, alpha, L, v, ws.base, cx);
    if (f.kind == FRAMES_YUV420)
        return launch_mark_verify_copies_yuv420(in, out, f.layout, copies, n, f0, cf, f.H, f.W, wm, n_wm, wm_rows, alpha, L, v, ws.base, cx);
    return fail(OFMK_E_ARG, "internal: no copies kernel for float32 frames%s");
}

// The read-out of cf frames' records.  counts / bits / soft are the call's arrays (any may be null) and these frames start at
// row `row` of them: f0, or q * n + f0 in copy q of a copies call.  counts were cleared by the kernel that wrote the records,
// soft by the call.  The hard outputs and the soft sums take a launch each: finalize's one LDS histogram serves the counts or
// the soft sums.
int read_out(const RecView &v, const FrameFmt &f, size_t row, int cf, int L, double alpha, int32_t *counts, uint8_t *bits,
             long long *soft, const Ctx &cx) {
    FinArgs a = fin_base(v, f.H, f.W, alpha);
    a.L = L;
    if (counts || bits) {
        a.counts = counts ? counts + row * L : nullptr;
        a.bits = bits ? bits + row * a.N : nullptr;
        if (int rc = launch_finalize(a, cf, cx)) return rc;
    }
    if (!soft) return OFMK_OK;
    a.counts = nullptr;
    a.bits = nullptr;
    a.soft = soft + row * L;
    return launch_finalize(a, cf, cx);
}

// analyze + mark of frames [f0, f0+cf) of the call; verify = also leave the marked frames' records in the workspace (fused
// kernel), ready for read_out(marked_records(ws)).  zero_counts: the call's [n][L] counts to clear for these frames, or null.
int embed_chunk(const FrameFmt &f, const uint8_t *in, uint8_t *out, int f0, int cf, const uint8_t *wm, int n_wm, const int32_t *wm_row,
                double alpha, const Workspace &ws, bool verify, const Ctx &cx, int32_t *zero_counts = nullptr, int L = 0) {
    const size_t fo = (size_t)f0 * f.frame_bytes;
    if (int rc = analyze_frames(f, in + fo, cf, ws, cx, zero_counts ? zero_counts + (size_t)f0 * L : nullptr, L)) return rc;
    return mark_frames(f, in + fo, out + fo, cf, wm, n_wm, wm_row ? wm_row + f0 : nullptr, alpha, ws, verify, cx);
}

// analyze + read-out of frames [f0, f0+cf) of `in` ([n] frames) into rows [f0, f0+cf) of counts / bits (hard; the analyze
// kernel clears the counts) or of soft (cleared by the call)
int detect_chunk(const FrameFmt &f, const uint8_t *in, int f0, int cf, int L, double alpha, int32_t *counts, uint8_t *bits,
                 long long *soft, const Workspace &ws, const Ctx &cx) {
    if (int rc = analyze_frames(f, in + (size_t)f0 * f.frame_bytes, cf, ws, cx, counts ? counts + (size_t)f0 * L : nullptr, L)) return rc;
    return read_out(input_records(ws), f, (size_t)f0, cf, L, alpha, counts, bits, soft, cx);
}

// The bodies of the entry points, one per call shape; the arguments are checked by the entry point, the workspace here.
int embed_frames(const FrameFmt &f, const uint8_t *in, uint8_t *out, int n, const uint8_t *wm, int n_wm, const int32_t *wm_row,
                 double alpha, int chunk_frames, void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts) {
    Workspace ws;
    if (int rc = carve(workspace, workspace_bytes, f.H, f.W, chunk_frames, ws)) return rc;
    const Ctx cx = make_ctx(stream, opts);
    return for_chunks(n, ws.frames, [&](int f0, int cf) { return embed_chunk(f, in, out, f0, cf, wm, n_wm, wm_row, alpha, ws, false, cx); });
}

// hard (counts and / or bits) or soft: one of the two per call
int detect_frames(const FrameFmt &f, const uint8_t *in, int n, int L, double alpha, int32_t *counts, uint8_t *bits, long long *soft,
                  int chunk_frames, void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts) {
    Workspace ws;
    if (int rc = carve(workspace, workspace_bytes, f.H, f.W, chunk_frames, ws)) return rc;
    const Ctx cx = make_ctx(stream, opts);
    // counts are cleared by each chunk's analyze kernel
    if (soft) HIP_TRY(launch_zero(soft, (size_t)n * L * sizeof(long long), cx.s));
    return for_chunks(n, ws.frames, [&](int f0, int cf) { return detect_chunk(f, in, f0, cf, L, alpha, counts, bits, soft, ws, cx); });
}

int embed_detect_frames(const FrameFmt &f, const uint8_t *in, uint8_t *out, int n, const uint8_t *wm, int n_wm, const int32_t *wm_row,
                        double alpha, int L, int32_t *counts, uint8_t *bits, int chunk_frames, void *workspace, size_t workspace_bytes,
                        void *stream, const ofmk_opts *opts) {
    Workspace ws;
    if (int rc = carve(workspace, workspace_bytes, f.H, f.W, chunk_frames, ws)) return rc;
    const Ctx cx = make_ctx(stream, opts);
    return for_chunks(n, ws.frames, [&](int f0, int cf) {
        if (!(cx.flags & OFMK_F_SEPARATE_DETECT)) {
            if (int rc = embed_chunk(f, in, out, f0, cf, wm, n_wm, wm_row, alpha, ws, true, cx, counts, L)) return rc;
            return read_out(marked_records(ws), f, (size_t)f0, cf, L, alpha, counts, bits, nullptr, cx);
        }
        if (int rc = embed_chunk(f, in, out, f0, cf, wm, n_wm, wm_row, alpha, ws, false, cx)) return rc;
        return detect_chunk(f, out, f0, cf, L, alpha, counts, bits, nullptr, ws, cx);
    });
}

int embed_copies_frames(const FrameFmt &f, const uint8_t *in, uint8_t *out, int copies, int n, const uint8_t *wm, int n_wm,
                        const int32_t *wm_rows, double alpha, int chunk_frames, void *workspace, size_t workspace_bytes, void *stream,
                        const ofmk_opts *opts) {
    Workspace ws;
    if (int rc = carve(workspace, workspace_bytes, f.H, f.W, chunk_frames, ws)) return rc;
    const Ctx cx = make_ctx(stream, opts);
    int rc = for_chunks(n, ws.frames, [&](int f0, int cf) {      // one analysis per chunk serves every copy
        if (int rc = analyze_frames(f, in + (size_t)f0 * f.frame_bytes, cf, ws, cx)) return rc;
        return mark_copies(f, in, out, copies, n, f0, cf, wm, n_wm, wm_rows, alpha, ws, cx);
    });
    if (rc) return rc;
    // pixels outside the 8x8 block grid: only interleaved RGB frames have any (planes come in multiples of 8), and nothing is launched without
    return launch_copy_fringe_copies(in, out, copies, n, f.H, f.W, cx.s);
}

// The copies-with-verify calls: counts / bits (the hard read-out of every copy) and / or soft (its int64 [copies][n][L] sums).
int embed_detect_copies_frames(const FrameFmt &f, const uint8_t *in, uint8_t *out, int copies, int n, const uint8_t *wm, int n_wm,
                               const int32_t *wm_rows, double alpha, int L, int32_t *counts, uint8_t *bits, long long *soft,
                               int chunk_frames, void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts) {
    CopiesWorkspace ws;
    if (int rc = carve_copies(workspace, workspace_bytes, copies, f.H, f.W, chunk_frames, ws)) return rc;
    const Ctx cx = make_ctx(stream, opts);
    const bool hard = counts || bits;
    const int nblk = (f.H / 8) * (f.W / 8);
    const size_t N = (size_t)((long long)f.H * f.W / 64);
    if (soft) HIP_TRY(launch_zero(soft, (size_t)copies * n * L * sizeof(long long), cx.s));
    int rc = for_chunks(n, ws.base.frames, [&](int f0, int cf) {      // one analysis of the input per chunk serves every copy
        if (int rc = analyze_frames(f, in + (size_t)f0 * f.frame_bytes, cf, ws.base, cx)) return rc;
        if (!(cx.flags & OFMK_F_SEPARATE_DETECT)) {
            if (int rc = mark_verify_copies(f, in, out, copies, n, f0, cf, wm, n_wm, wm_rows, alpha, L, counts, ws, cx)) return rc;
            for (int q = 0; q < copies; ++q)                      // the small launches per copy on the records the fused launch left
                if (int rc = read_out(copy_records(ws, q, nblk), f, (size_t)q * n + f0, cf, L, alpha, counts, bits, soft, cx)) return rc;
            return (int)OFMK_OK;
        }
        // the literal sequence: mark every copy, then detect (and soft-detect) each written copy (its analysis overwrites the
        // input's records, which the chunk's mark launch, earlier in the stream, has already used)
        if (int rc = mark_copies(f, in, out, copies, n, f0, cf, wm, n_wm, wm_rows, alpha, ws.base, cx)) return rc;
        for (int q = 0; q < copies; ++q) {
            const uint8_t *out_q = out + (size_t)q * n * f.frame_bytes;
            if (hard)
                if (int rc = detect_chunk(f, out_q, f0, cf, L, alpha, counts ? counts + (size_t)q * n * L : nullptr,
                                          bits ? bits + (size_t)q * n * N : nullptr, nullptr, ws.base, cx)) return rc;
            if (soft)
                if (int rc = detect_chunk(f, out_q, f0, cf, L, alpha, nullptr, nullptr, soft + (size_t)q * n * L, ws.base, cx)) return rc;
        }
        return (int)OFMK_OK;
    });
    if (rc) return rc;
    return launch_copy_fringe_copies(in, out, copies, n, f.H, f.W, cx.s);      // as in embed_copies_frames
}

// ---- block-grid resync of cropped leaks, both codecs (resync_kernels.hiph, dct_resync_kernels.hiph, planar_resync_kernels.hiph;
// build extensions, not reference semantics) ---------------------------------------------------------------------------------
// What the frames of a resync call are, as FrameFmt is for the DCT codec's call path: an entry point checks its own arguments,
// makes this value and calls one of the four bodies below (svd_sync_scores, svd_soft_window, sync_scores, soft_window).  Only the
// leaf launchers -- the functions that build a kernel's geometry and name the kernel -- ask which format they have.
enum LeakKind { LEAK_RGB8, LEAK_YUV420 };
struct LeakFmt {
    LeakKind kind;
    int layout;            // LEAK_YUV420: OFMK_YUV_I420 / OFMK_YUV_NV12
    int H, W;              // any values >= 8; even on planes (check_leak)
    size_t frame_bytes;
    int phases;            // grid phases the search sums: all 64, or the 16 with even py and px on planes
};
LeakFmt rgb8_leak(int H, int W) { return {LEAK_RGB8, 0, H, W, (size_t)H * W * 3, 64}; }
LeakFmt yuv420_leak(int layout, int H, int W) { return {LEAK_YUV420, layout, H, W, (size_t)H * W * 3 / 2, 16}; }

// What planes ask on top of interleaved frames: a known layout and EVEN H and W.  No multiple of 8 and no alignment: the kernels
// load bytes.
int check_leak(const LeakFmt &f) {
    if (f.kind != LEAK_YUV420) return OFMK_OK;
    if (f.layout != OFMK_YUV_I420 && f.layout != OFMK_YUV_NV12) return fail(OFMK_E_ARG, "layout must be OFMK_YUV_I420 or OFMK_YUV_NV12%s");
    if (f.H % 2 || f.W % 2) return fail(OFMK_E_ARG, "4:2:0 planes need even H and W%s");
    return OFMK_OK;
}

// the window calls' checks (both codecs); rows / cols: the window's units
int check_window(const LeakFmt &f, int py, int px, int canvas_cols, int base, int &rows, int &cols) {
    if (py < 0 || py > 7 || px < 0 || px > 7) return fail(OFMK_E_ARG, "the phase (py, px) must be in 0..7%s");
    if (f.kind == LEAK_YUV420 && (py % 2 || px % 2))
        return fail(OFMK_E_ARG, "an odd phase does not exist on 4:2:0 planes: py and px must be even%s");
    rows = (f.H - py) / 8;
    cols = (f.W - px) / 8;
    if (rows < 1 || cols < 1) return fail(OFMK_E_ARG, "no full 8x8 unit at this phase%s");
    if (canvas_cols < cols) return fail(OFMK_E_ARG, "canvas_cols is smaller than the window's units per row%s");
    if (base < 0) return fail(OFMK_E_ARG, "base must not be negative%s");
    if ((long long)base + (long long)rows * canvas_cols >= (1LL << 31)) return fail(OFMK_E_ARG, "base + rows * canvas_cols must be < 2^31%s");
    return OFMK_OK;
}

int check_alpha(double alpha) {
    if (!(alpha > 0.0) || !(alpha <= 1.79769313486231570815e308)) return fail(OFMK_E_ARG, "alpha must be a positive finite number%s");
    return OFMK_OK;
}

PlaneGeom make_plane_geom(const LeakFmt &f) {
    PlaneGeom p;
    p.H = f.H;
    p.W = f.W;
    p.cpitch = f.layout == OFMK_YUV_I420 ? f.W / 2 : f.W;
    p.cstep = f.layout == OFMK_YUV_I420 ? 1 : 2;
    p.frame_stride = f.frame_bytes;
    p.u_off = (size_t)f.H * f.W;
    p.v_off = f.layout == OFMK_YUV_I420 ? p.u_off + (size_t)f.H * f.W / 4 : p.u_off + 1;
    return p;
}

PWinGeom make_window_geom(const LeakFmt &f, int rows, int cols, int frames) {
    PWinGeom g;
    g.p = make_plane_geom(f);
    g.wb = cols;
    g.nblk = rows * cols;
    g.inv_wb = 1.0f / (float)cols;
    g.frames = frames;
    return g;
}

// -- DwtDctSvd: no workspace, one launch per chunk of at most kMaxChunk frames --
// leaf: the phase scores of cf frames from `first` into `scores` ([cf][64])
void launch_svd_sync_scores(const LeakFmt &f, const uint8_t *first, int cf, float scale, unsigned long long *scores, const Ctx &cx) {
    ScopedTiming timing(KIND_SVD, cx);
    if (f.kind == LEAK_YUV420) {
        PSyncGeom g;
        g.p = make_plane_geom(f);
        g.Hc = f.H / 2;
        g.Wc = f.W / 2;
        g.rects_x = (g.Wc - 3 + kPsRect * kPsStrip - 1) / (kPsRect * kPsStrip);
        g.scale = scale;
        const unsigned rects = (unsigned)(g.rects_x * ((g.Hc - 3 + kPsRect - 1) / kPsRect));
        OFMK_TIMED_LAUNCH(timing, svd_sync_scores_yuv420_kernel, dim3(rects, (unsigned)cf), dim3(kThreads), 0, cx.s, first, g, scores);
        return;
    }
    SyncGeom g;
    g.H = f.H;
    g.W = f.W;
    g.rects_x = (f.W - 7 + kSyncRect * kSyncStrip - 1) / (kSyncRect * kSyncStrip);
    g.rects = g.rects_x * ((f.H - 7 + kSyncRect - 1) / kSyncRect);
    g.frame_stride = f.frame_bytes;
    g.scale = scale;
    OFMK_TIMED_LAUNCH(timing, svd_sync_scores_rgb8_kernel, dim3((unsigned)g.rects, (unsigned)cf), dim3(kThreads), 0, cx.s, first, g, scores);
}

// leaf: the window read-out of cf frames from `first`; w.soft is these frames' [cf][L]
void launch_svd_soft_window(const LeakFmt &f, const uint8_t *first, int cf, int rows, int cols, const WindowArgs &w, const Ctx &cx) {
    ScopedTiming timing(KIND_SVD, cx);
    if (f.kind == LEAK_YUV420) {
        const PWinGeom g = make_window_geom(f, rows, cols, cf);
        OFMK_TIMED_LAUNCH(timing, svd_soft_window_yuv420_kernel, xcd_grid(g.nblk, cf), dim3(kThreads), 0, cx.s, first, g, w);
        return;
    }
    Geom g = svd_geom(f.H, f.W);             // the frame's W and stride ...
    g.wb = cols;                             // ... with the window's units
    g.inv_wb = 1.0f / (float)cols;
    g.nblk = rows * cols;
    g.frames = cf;
    OFMK_TIMED_LAUNCH(timing, svd_soft_window_rgb8_kernel, xcd_grid(g.nblk, cf), dim3(kThreads), 0, cx.s, first, g, w);
}

// in, scores: checked by the entry point
int svd_sync_scores(const LeakFmt &f, const uint8_t *in, int n, const double *scales, int blk, long long *scores, void *stream,
                    const ofmk_opts *opts) {
    if (int rc = check_leak(f)) return rc;
    SvdArgs a;
    if (int rc = check_resync_scales(a, scales, blk, true)) return rc;
    const Ctx cx = make_ctx(stream, opts);
    HIP_TRY(launch_zero(scores, (size_t)n * 64 * sizeof(long long), cx.s));
    for_chunks(n, kMaxChunk, [&](int f0, int cf) {
        launch_svd_sync_scores(f, in + (size_t)f0 * f.frame_bytes, cf, a.scales[1], reinterpret_cast<unsigned long long *>(scores) + (size_t)f0 * 64,
                               cx);
        return OFMK_OK;
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// in, n, H, W, L, soft: checked by the entry point (check_soft_args)
int svd_soft_window(const LeakFmt &f, const uint8_t *in, int n, int py, int px, int canvas_cols, int base, int L, const double *scales,
                    int blk, long long *soft, void *stream, const ofmk_opts *opts) {
    if (int rc = check_leak(f)) return rc;
    int rows, cols;
    if (int rc = check_window(f, py, px, canvas_cols, base, rows, cols)) return rc;
    SvdArgs sa;
    if (int rc = check_resync_scales(sa, scales, blk, false)) return rc;
    const Ctx cx = make_ctx(stream, opts);
    HIP_TRY(launch_zero(soft, (size_t)n * L * sizeof(long long), cx.s));
    if (!(sa.scales[1] > 0.f)) return OFMK_OK;
    for_chunks(n, kMaxChunk, [&](int f0, int cf) {
        const WindowArgs w{py, px, canvas_cols, base, L, sa.scales[1], soft + (size_t)f0 * L};
        launch_svd_soft_window(f, in + (size_t)f0 * f.frame_bytes, cf, rows, cols, w, cx);
        return OFMK_OK;
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// -- the DCT codec: two passes over records in the caller's workspace, chunks of what it holds --
// Workspace of the dense phase search: per frame in flight one record (kRec floats) per origin searched -- every pixel origin
// of interleaved frames, every EVEN one of planes -- and the per-phase sums.
struct SyncWorkspace {
    float *rec;                  // kRec planes of [frames][norig]
    unsigned long long *sums;    // [frames][phases]
    int frames;                  // chunk capacity
    size_t norig;
};
size_t sync_origins(const LeakFmt &f) {
    return f.kind == LEAK_YUV420 ? (size_t)(f.H / 2 - 3) * (f.W / 2 - 3) : (size_t)(f.H - 7) * (f.W - 7);
}
size_t sync_per_frame_bytes(const LeakFmt &f) { return sync_origins(f) * kRec * sizeof(float) + f.phases * sizeof(unsigned long long); }

int carve_sync(void *ws, size_t bytes, const LeakFmt &f, int want_frames, SyncWorkspace &out) {
    if (!ws) return fail(OFMK_E_ARG, "workspace is null%s");
    if ((uintptr_t)ws % 256) return fail(OFMK_E_ARG, "workspace must be 256-byte aligned%s");
    const size_t per = sync_per_frame_bytes(f);
    if (bytes < per + kFixedBytes)
        return fail(OFMK_E_WORKSPACE, "workspace smaller than %s(1, H, W)",
                    f.kind == LEAK_YUV420 ? "ofmk_sync_workspace_bytes_yuv420" : "ofmk_sync_workspace_bytes");
    size_t cap = (bytes - kFixedBytes) / per;
    if (want_frames > 0 && (size_t)want_frames < cap) cap = want_frames;
    if (cap > (size_t)kMaxChunk) cap = kMaxChunk;
    out.frames = (int)cap;
    out.norig = sync_origins(f);
    out.rec = static_cast<float *>(ws);
    out.sums = reinterpret_cast<unsigned long long *>(static_cast<char *>(ws) + align256(cap * out.norig * kRec * sizeof(float)));
    return OFMK_OK;
}

// leaf: analyse every origin of cf frames from `first` (timed as the format's analyze), then score every origin under its
// phase's mean into `scores` ([cf][64]; timed as finalize)
void launch_sync_passes(const LeakFmt &f, const uint8_t *first, int cf, double alpha, unsigned long long *scores, const SyncWorkspace &ws,
                        const Ctx &cx) {
    if (f.kind == LEAK_YUV420) {
        PDctSyncGeom g;
        g.p = make_plane_geom(f);
        g.oh = f.H / 2 - 3;
        g.ow = f.W / 2 - 3;
        g.rects_x = (g.ow + kPdRectX * kPdStrip - 1) / (kPdRectX * kPdStrip);
        g.norig = ws.norig;
        g.plane = (size_t)ws.frames * ws.norig;
        const dim3 grid((unsigned)(g.rects_x * ((g.oh + kPdRectY - 1) / kPdRectY)), (unsigned)cf);
        {
            ScopedTiming timing(KIND_PLANAR_ANALYZE, cx);
            OFMK_TIMED_LAUNCH(timing, dct_sync_analyze_yuv420_kernel, grid, dim3(kThreads), 0, cx.s, first, g, ws.rec, ws.sums);
        }
        ScopedTiming timing(KIND_FINALIZE, cx);
        OFMK_TIMED_LAUNCH(timing, dct_sync_scores_yuv420_kernel, grid, dim3(kThreads), 0, cx.s, g, ws.rec, ws.sums, alpha, scores);
        return;
    }
    DctSyncGeom g;
    g.H = f.H;
    g.W = f.W;
    g.ow = f.W - 7;
    g.rects_x = (f.W - 7 + kDsRect * kDsStrip - 1) / (kDsRect * kDsStrip);
    g.frame_stride = f.frame_bytes;
    g.norig = ws.norig;
    g.plane = (size_t)ws.frames * ws.norig;
    const dim3 grid((unsigned)(g.rects_x * ((f.H - 7 + kDsRect - 1) / kDsRect)), (unsigned)cf);
    {
        ScopedTiming timing(KIND_ANALYZE, cx);
        OFMK_TIMED_LAUNCH(timing, dct_sync_analyze_rgb8_kernel, grid, dim3(kThreads), 0, cx.s, first, g, ws.rec, ws.sums);
    }
    ScopedTiming timing(KIND_FINALIZE, cx);
    OFMK_TIMED_LAUNCH(timing, dct_sync_scores_kernel, grid, dim3(kThreads), 0, cx.s, g, ws.rec, ws.sums, alpha, scores);
}

// leaf: the window's records into ws -- the window's blocks read through the frame's own pitch and stride; ws was carved for
// them (8 rows x 8 cols pixels)
int launch_window_analyze(const LeakFmt &f, const uint8_t *first, int cf, int py, int px, int rows, int cols, const Workspace &ws,
                          const Ctx &cx) {
    if (f.kind == LEAK_YUV420) {
        // the grid's x extent is the tile count emit_block files the per-tile sums under, and it is ws.tiles (both are
        // ceil(nblk / kThreads))
        const PWinGeom g = make_window_geom(f, rows, cols, cf);
        const dim3 grid = grid_2d(g.nblk, cf);
        if ((int)grid.x != ws.tiles) return fail(OFMK_E_ARG, "internal: tile count of the launch and of the workspace differ%s");
        ScopedTiming timing(KIND_PLANAR_ANALYZE, cx);
        OFMK_TIMED_LAUNCH(timing, analyze_window_yuv420_kernel, grid, dim3(kThreads), 0, cx.s, first, g, py, px, ws.plane, ws.rec, ws.ysum);
        return OFMK_OK;
    }
    Geom g = make_geom(8 * rows, 8 * cols, ws, cf);
    g.W = f.W;
    g.frame_stride = f.frame_bytes;
    ScopedTiming timing(KIND_ANALYZE, cx);
    OFMK_TIMED_LAUNCH(timing, (analyze_kernel<SRC_RGB8, false>), xcd_grid(g.nblk, cf), dim3(kThreads), 0, cx.s,
                      static_cast<const void *>(first + ((size_t)py * f.W + px) * 3), g, ws.rec, ws.ysum, static_cast<int32_t *>(nullptr), 0);
    return OFMK_OK;
}

// in, scores: checked by the entry point
int sync_scores(const LeakFmt &f, const uint8_t *in, int n, double alpha, long long *scores, int chunk_frames, void *workspace,
                size_t workspace_bytes, void *stream, const ofmk_opts *opts) {
    if (int rc = check_leak(f)) return rc;
    if (int rc = check_alpha(alpha)) return rc;
    SyncWorkspace ws;
    if (int rc = carve_sync(workspace, workspace_bytes, f, chunk_frames, ws)) return rc;
    const Ctx cx = make_ctx(stream, opts);
    HIP_TRY(launch_zero(scores, (size_t)n * 64 * sizeof(long long), cx.s));
    return for_chunks(n, ws.frames, [&](int f0, int cf) {
        HIP_TRY(launch_zero(ws.sums, (size_t)cf * f.phases * sizeof(unsigned long long), cx.s));
        launch_sync_passes(f, in + (size_t)f0 * f.frame_bytes, cf, alpha, reinterpret_cast<unsigned long long *>(scores) + (size_t)f0 * 64, ws,
                           cx);
        HIP_TRY(hipGetLastError());
        return (int)OFMK_OK;
    });
}

// in, n, H, W, L, soft: checked by the entry point (check_soft_args).  Per chunk: the analyze on the window, then the soft
// finalize with canvas positions (timed as finalize).
int soft_window(const LeakFmt &f, const uint8_t *in, int n, int py, int px, int canvas_cols, int base, int L, double alpha, long long *soft,
                int chunk_frames, void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts) {
    if (int rc = check_leak(f)) return rc;
    if (int rc = check_alpha(alpha)) return rc;
    int rows, cols;
    if (int rc = check_window(f, py, px, canvas_cols, base, rows, cols)) return rc;
    Workspace ws;
    if (int rc = carve(workspace, workspace_bytes, 8 * rows, 8 * cols, chunk_frames, ws)) return rc;
    const Ctx cx = make_ctx(stream, opts);
    HIP_TRY(launch_zero(soft, (size_t)n * L * sizeof(long long), cx.s));
    DctWindowArgs a;
    a.rec = ws.rec;
    a.plane = ws.plane;
    a.ysum = ws.ysum;
    a.tiles = ws.tiles;
    a.nblk = rows * cols;
    a.cols = cols;
    a.canvas_cols = canvas_cols;
    a.base = base;
    a.L = L;
    a.alpha = alpha;
    const int per_wg = kThreads * kFinItems;
    return for_chunks(n, ws.frames, [&](int f0, int cf) {
        if (int rc = launch_window_analyze(f, in + (size_t)f0 * f.frame_bytes, cf, py, px, rows, cols, ws, cx)) return rc;
        a.soft = soft + (size_t)f0 * L;
        {
            ScopedTiming timing(KIND_FINALIZE, cx);
            OFMK_TIMED_LAUNCH(timing, finalize_soft_window_kernel, dim3((unsigned)((a.nblk + per_wg - 1) / per_wg), (unsigned)cf),
                              dim3(kThreads), 0, cx.s, a);
        }
        HIP_TRY(hipGetLastError());
        return (int)OFMK_OK;
    });
}

// The residuals and the moments share arguments, checks, tiles and chunks; WORDS int64 per leak frame and source, cleared here.
template <auto Kernel, int WORDS>
int align_window_sums(const uint8_t *lib, int N, const uint8_t *leak, int m, int h, int w, int H, int W, const int32_t *first, int span,
                             const ofmk_affine *geom, long long *res, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    if (int rc = check_dims(m, H, W)) return rc;
    if (N < 1) return fail(OFMK_E_ARG, "N must be at least 1%s");
    if (H > kAlignMaxSide || W > kAlignMaxSide) return fail(OFMK_E_ARG, "canvas H, W must be at most 4096%s");
    if (int rc = check_leak_dims(h, w)) return rc;
    if (span < 1 || span > kResidualMaxSpan) return fail(OFMK_E_ARG, "span must be in [1, 16]%s");
    if (!lib || !leak || !first || !geom || !res) return fail(OFMK_E_ARG, "null pointer%s");
    ResidualArgs a;
    if (int rc = check_map(geom, a.m)) return rc;
    const Ctx cx = make_ctx(stream, opts);
    HIP_TRY(launch_zero(res, (size_t)m * span * WORDS * sizeof(long long), cx.s));
    a.h = h; a.w = w; a.H = H; a.W = W;
    a.tiles_x = (W + kAlignTile - 1) / kAlignTile;
    a.N = N; a.span = span;
    a.leak_stride = (size_t)h * w * 3;
    a.src_stride = (size_t)H * W * 3;
    const int tiles = a.tiles_x * ((H + kAlignTile - 1) / kAlignTile);          // at most 64 * 64
    for_chunks(m, kMaxChunk, [&](int f0, int cf) {
        ScopedTiming timing(KIND_SVD, cx);
        OFMK_TIMED_LAUNCH(timing, Kernel, dim3((unsigned)tiles, (unsigned)cf), dim3(kThreads), 0, cx.s, lib,
                          leak + (size_t)f0 * a.leak_stride, first + f0, a, reinterpret_cast<unsigned long long *>(res) + (size_t)f0 * span * WORDS);
        return OFMK_OK;
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

}  // namespace

extern "C" {

int ofmk_version(void) { return OFMK_ABI_VERSION; }
const char *ofmk_last_error(void) { return g_err; }

size_t ofmk_workspace_bytes(int frames_in_flight, int H, int W) {
    if (frames_in_flight < 1 || H < 8 || W < 8) return 0;
    return per_frame_bytes(H, W) * (size_t)frames_in_flight + kFixedBytes;
}

int ofmk_embed_rgb8(const uint8_t *in, uint8_t *out, int n, int H, int W, const uint8_t *wm, int n_wm,
                    const int32_t *wm_row, double alpha, int chunk_frames, void *workspace, size_t workspace_bytes,
                    void *stream, const ofmk_opts *opts) {
    if (int rc = check_opts(opts)) return rc;
    if (int rc = check_embed_args(in, out, n, H, W, wm, n_wm)) return rc;
    return embed_frames(rgb8_frames(H, W), in, out, n, wm, n_wm, wm_row, alpha, chunk_frames, workspace, workspace_bytes, stream, opts);
}

int ofmk_detect_rgb8(const uint8_t *in, int n, int H, int W, int L, double alpha, int32_t *counts, uint8_t *bits,
                     int chunk_frames, void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts) {
    if (int rc = check_opts(opts)) return rc;
    if (int rc = check_detect_args(in, n, H, W, L, counts, bits)) return rc;
    return detect_frames(rgb8_frames(H, W), in, n, L, alpha, counts, bits, nullptr, chunk_frames, workspace, workspace_bytes, stream, opts);
}

// Build extension, not reference semantics: per payload position the sum over the frame's blocks
// of -cos(pi * C21/step) in 2^14 fixed point (positive = the position reads as 1).  One histogram per call, so
// it is a separate entry point from the hard-decision counts.
int ofmk_detect_soft_rgb8(const uint8_t *in, int n, int H, int W, int L, double alpha, long long *soft, int chunk_frames,
                          void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts) {
    if (int rc = check_opts(opts)) return rc;
    if (int rc = check_soft_args(in, n, H, W, L, soft)) return rc;
    return detect_frames(rgb8_frames(H, W), in, n, L, alpha, nullptr, nullptr, soft, chunk_frames, workspace, workspace_bytes, stream, opts);
}

int ofmk_embed_detect_rgb8(const uint8_t *in, uint8_t *out, int n, int H, int W, const uint8_t *wm, int n_wm,
                           const int32_t *wm_row, double alpha, int L, int32_t *counts, uint8_t *bits,
                           int chunk_frames, void *workspace, size_t workspace_bytes, void *stream,
                           const ofmk_opts *opts) {
    if (int rc = check_opts(opts)) return rc;
    if (int rc = check_embed_args(in, out, n, H, W, wm, n_wm)) return rc;
    if (int rc = check_detect_args(out, n, H, W, L, counts, bits)) return rc;
    return embed_detect_frames(rgb8_frames(H, W), in, out, n, wm, n_wm, wm_row, alpha, L, counts, bits, chunk_frames, workspace,
                               workspace_bytes, stream, opts);
}

int ofmk_encode_yuv32f(float *yuv, int n, int H, int W, const uint8_t *wm, int n_wm, const int32_t *wm_row,
                       double alpha, int chunk_frames, void *workspace, size_t workspace_bytes, void *stream,
                       const ofmk_opts *opts) {
    if (int rc = check_opts(opts)) return rc;
    if (int rc = check_embed_args(yuv, yuv, n, H, W, wm, n_wm)) return rc;
    uint8_t *p = reinterpret_cast<uint8_t *>(yuv);
    return embed_frames(yuv32f_frames(H, W), p, p, n, wm, n_wm, wm_row, alpha, chunk_frames, workspace, workspace_bytes, stream, opts);
}

int ofmk_decode_yuv32f(const float *yuv, int n, int H, int W, int L, double alpha, int32_t *counts, uint8_t *bits,
                       int chunk_frames, void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts) {
    if (int rc = check_opts(opts)) return rc;
    if (int rc = check_detect_args(yuv, n, H, W, L, counts, bits)) return rc;
    return detect_frames(yuv32f_frames(H, W), reinterpret_cast<const uint8_t *>(yuv), n, L, alpha, counts, bits, nullptr, chunk_frames,
                         workspace, workspace_bytes, stream, opts);
}

int ofmk_debug_planes(const void *frame, int src_is_yuv32f, int H, int W, double alpha, const uint8_t *wm,
                      float *y_dc, double *lum_mask, double *tex_mask, double *step, float *c21_pre,
                      float *c21_post, void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    int rc = check_dims(1, H, W);
    if (rc) return rc;
    if (!frame) return fail(OFMK_E_ARG, "null frame pointer%s");
    if (c21_post && !wm) return fail(OFMK_E_ARG, "c21_post requested without a watermark%s");
    Workspace ws;
    if ((rc = carve(workspace, workspace_bytes, H, W, 1, ws))) return rc;
    const Ctx cx = make_ctx(stream, opts);
    const FrameFmt f = src_is_yuv32f ? yuv32f_frames(H, W) : rgb8_frames(H, W);
    if ((rc = analyze_frames(f, static_cast<const uint8_t *>(frame), 1, ws, cx))) return rc;
    FinArgs a = fin_base(input_records(ws), H, W, alpha);
    a.wm = wm;
    a.y_dc = y_dc;
    a.lum = lum_mask;
    a.tex = tex_mask;
    a.step = step;
    a.c21_pre = c21_pre;
    a.c21_post = wm ? c21_post : nullptr;
    return launch_finalize(a, 1, cx);
}

int ofmk_stage_analyze_rgb8(const uint8_t *in, int n, int H, int W, void *workspace, size_t workspace_bytes,
                            void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    int rc = check_dims(n, H, W);
    if (rc) return rc;
    if (!in) return fail(OFMK_E_ARG, "null frame pointer%s");
    Workspace ws;
    if ((rc = carve(workspace, workspace_bytes, H, W, n, ws))) return rc;
    if (ws.frames < n) return fail(OFMK_E_WORKSPACE, "stage call needs workspace for all n frames%s");
    return analyze_frames(rgb8_frames(H, W), in, n, ws, make_ctx(stream, opts));
}

int ofmk_stage_mark_rgb8(const uint8_t *in, uint8_t *out, int n, int H, int W, const uint8_t *wm, double alpha,
                         int fused, void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    int rc = check_embed_args(in, out, n, H, W, wm, 1);
    if (rc) return rc;
    Workspace ws;
    if ((rc = carve(workspace, workspace_bytes, H, W, n, ws))) return rc;
    if (ws.frames < n) return fail(OFMK_E_WORKSPACE, "stage call needs workspace for all n frames%s");
    return mark_frames(rgb8_frames(H, W), in, out, n, wm, 1, nullptr, alpha, ws, fused != 0, make_ctx(stream, opts));
}

int ofmk_svd_embed_rgb8(const uint8_t *in, uint8_t *out, int n, int H, int W, const uint8_t *wm, int n_wm,
                        const int32_t *wm_row, const double *scales, int blk, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    int rc = check_embed_args(in, out, n, H, W, wm, n_wm);
    if (rc) return rc;
    if ((rc = check_blk(blk))) return rc;
    SvdArgs a;
    if ((rc = make_svd_args(a, H, W, scales, false, wm, n_wm, wm_row, 1, nullptr, nullptr, nullptr))) return rc;
    return launch_svd_rgb8(in, out, n, H, W, SVD_EMBED, blk, a, make_ctx(stream, opts));
}

// scales[1] <= 0: zeroed counts / bits (zero_svd_readout)
int ofmk_svd_detect_rgb8(const uint8_t *in, int n, int H, int W, int L, const double *scales, int blk, int32_t *counts, uint8_t *bits,
                         void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    int rc = check_detect_args(in, n, H, W, L, counts, bits);
    if (rc) return rc;
    if ((rc = check_blk(blk))) return rc;
    SvdArgs a;
    if ((rc = make_svd_args(a, H, W, scales, true, nullptr, 0, nullptr, L, counts, bits, opts))) return rc;
    if (!(a.scales[1] > 0.f)) return zero_svd_readout(n, H, W, blk, a, static_cast<hipStream_t>(stream));
    return launch_svd_rgb8(in, nullptr, n, H, W, SVD_DETECT, blk, a, make_ctx(stream, opts));
}

// Build extension, not reference semantics: per payload position the sum over the frame's units of svd_soft_metric
// (svd_kernels.hiph), int64 [n][L], cleared here whatever it held.  scales[1] <= 0: all zeros, as the hard read-out.
int ofmk_svd_detect_soft_rgb8(const uint8_t *in, int n, int H, int W, int L, const double *scales, int blk, long long *soft,
                              void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    int rc = check_soft_args(in, n, H, W, L, soft);
    if (rc) return rc;
    if ((rc = check_blk(blk))) return rc;
    return svd_detect_soft(n, H, W, L, scales, soft, stream, [&](const SvdArgs &a) {
        return launch_svd_rgb8(in, nullptr, n, H, W, SVD_DETECT_SOFT, blk, a, make_ctx(stream, opts));
    });
}

// Build extension, not reference semantics (resync_kernels.hiph): scores[f][8 py + px] = sum of |svd_soft_metric| over the full 8x8
// windows of frame f at grid phase (py, px); int64 [n][64], cleared here whatever it held.  H, W: any values >= 8.
int ofmk_svd_sync_scores_rgb8(const uint8_t *in, int n, int H, int W, const double *scales, int blk, long long *scores, void *stream,
                              const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    if (int rc = check_dims(n, H, W)) return rc;
    if (!in || !scores) return fail(OFMK_E_ARG, "null pointer%s");
    return svd_sync_scores(rgb8_leak(H, W), in, n, scales, blk, scores, stream, opts);
}

// Build extension, not reference semantics (resync_kernels.hiph): the soft read-out of the units at grid phase (py, px) -- unit (i, j)
// is the 8x8 block at pixel (py + 8i, px + 8j) -- added into position (base + i * canvas_cols + j) mod L; int64 [n][L], cleared here.
// py = px = 0, canvas_cols = W / 8, base = 0 on frames with H, W multiples of 8: ofmk_svd_detect_soft_rgb8, integer for integer.
// scales[1] <= 0: all zeros, as that call.
int ofmk_svd_detect_soft_window_rgb8(const uint8_t *in, int n, int H, int W, int py, int px, int canvas_cols, int base, int L,
                                     const double *scales, int blk, long long *soft, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    if (int rc = check_soft_args(in, n, H, W, L, soft)) return rc;
    return svd_soft_window(rgb8_leak(H, W), in, n, py, px, canvas_cols, base, L, scales, blk, soft, stream, opts);
}

// ---- rescaled leaks (warp_kernels.hiph; build extensions, not reference semantics) ---------------------------------------------
// Host only: the counting rectangle of canvas units, out = {i0, i1, j0, j1}, all 0 when no unit counts.
int ofmk_warp_units(int h, int w, int H, int W, const ofmk_warp *geom, int out[4]) {
    return map_units<WarpMap>(h, w, H, W, geom, out);
}

// The leak resampled onto the canvas rectangle [oy, oy + Hout) x [ox, ox + Wout): u8 [n][Hout][Wout][3], every byte written.
int ofmk_warp_rgb8(const uint8_t *in, int n, int h, int w, uint8_t *out, int Hout, int Wout, int oy, int ox, const ofmk_warp *geom,
                   void *stream, const ofmk_opts *opts) {
    return warp_frames<WarpArgs, warp_rgb8_kernel, false>(in, n, h, w, out, Hout, Wout, oy, ox, geom, stream, opts);
}

// scores[f][k] = sum of |unit metric| over the counting units of frame f warped by cands[k] (DEVICE memory, [K]); int64 [n][K],
// cleared here whatever it held.  Candidates sit in gridDim.y and frames in gridDim.z, both in chunks of at most 65535.
int ofmk_svd_warp_scores_rgb8(const uint8_t *in, int n, int h, int w, int H, int W, const ofmk_warp *cands, int K, const double *scales,
                              int blk, long long *scores, void *stream, const ofmk_opts *opts) {
    if (int rc = check_search_args(opts, n, h, w, H, W, in && cands && scores, K)) return rc;
    SvdArgs sa;
    if (int rc = check_resync_scales(sa, scales, blk, true)) return rc;
    const Ctx cx = make_ctx(stream, opts);
    HIP_TRY(launch_zero(scores, (size_t)n * K * sizeof(long long), cx.s));
    WarpScoreArgs a;
    a.h = h; a.w = w;
    a.rows = H / 8; a.cols = W / 8;
    a.tiles_x = (a.cols + kWarpTileW - 1) / kWarpTileW;
    a.K = K;
    a.frame_stride = (size_t)h * w * 3;
    a.scale = sa.scales[1];
    const long long tiles = (long long)a.tiles_x * ((a.rows + kWarpTileH - 1) / kWarpTileH);
    const WarpMap *dc = reinterpret_cast<const WarpMap *>(cands);
    for_cand_frame_chunks(tiles, K, n, [&](int k0, int ck, int f0, int cf) {
        ScopedTiming timing(KIND_SVD, cx);
        OFMK_TIMED_LAUNCH(timing, svd_warp_scores_rgb8_kernel, dim3((unsigned)tiles, (unsigned)ck, (unsigned)cf), dim3(kThreads), 0, cx.s,
                          in + (size_t)f0 * a.frame_stride, dc + k0, a, reinterpret_cast<unsigned long long *>(scores) + (size_t)f0 * K + k0);
        return OFMK_OK;
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// The soft read-out of the counting units of the leak warped by *geom (HOST memory), unit (i, j) into position (i * (W / 8) + j) mod L;
// int64 [n][L], cleared here.  scales[1] <= 0 or no counting unit: all zeros.
int ofmk_svd_detect_soft_warp_rgb8(const uint8_t *in, int n, int h, int w, int H, int W, const ofmk_warp *geom, int L, const double *scales,
                                   int blk, long long *soft, void *stream, const ofmk_opts *opts) {
    return svd_detect_soft_mapped<WarpReadArgs, svd_soft_warp_rgb8_kernel>(in, n, h, w, H, W, geom, L, scales, blk, soft, stream, opts);
}

// ---- rotated leaks (affine_kernels.hiph; build extensions, not reference semantics) --------------------------------------------
// Host only: out = {i0, i1, j0, j1, count}, the bounding rectangle of the counting canvas units and their number; all 0 when none counts.
int ofmk_affine_units(int h, int w, int H, int W, const ofmk_affine *geom, int out[5]) {
    return map_units<AffineMap>(h, w, H, W, geom, out);
}

// The leak resampled onto the canvas rectangle [oy, oy + Hout) x [ox, ox + Wout): u8 [n][Hout][Wout][3], every byte written.
int ofmk_warp_affine_rgb8(const uint8_t *in, int n, int h, int w, uint8_t *out, int Hout, int Wout, int oy, int ox, const ofmk_affine *geom,
                          void *stream, const ofmk_opts *opts) {
    return warp_frames<AffineWarpArgs, warp_affine_rgb8_kernel, true>(in, n, h, w, out, Hout, Wout, oy, ox, geom, stream, opts);
}

// scores[f][k] = sum of |unit metric| over the counting units of frame f warped by cands[k] (DEVICE memory, [K]); int64 [n][K],
// cleared here whatever it held.  Candidates sit in gridDim.y and frames in gridDim.z, both in chunks of at most 65535.
int ofmk_svd_affine_scores_rgb8(const uint8_t *in, int n, int h, int w, int H, int W, const ofmk_affine *cands, int K, const double *scales,
                                int blk, long long *scores, void *stream, const ofmk_opts *opts) {
    if (int rc = check_search_args(opts, n, h, w, H, W, in && cands && scores, K)) return rc;
    SvdArgs sa;
    if (int rc = check_resync_scales(sa, scales, blk, true)) return rc;
    const Ctx cx = make_ctx(stream, opts);
    HIP_TRY(launch_zero(scores, (size_t)n * K * sizeof(long long), cx.s));
    AffineScoreArgs a;
    a.h = h; a.w = w;
    a.rows = H / 8; a.cols = W / 8;
    a.tiles_x = (a.cols + kAffineTile - 1) / kAffineTile;
    a.K = K;
    a.frame_stride = (size_t)h * w * 3;
    a.scale = sa.scales[1];
    const long long tiles = (long long)a.tiles_x * ((a.rows + kAffineTile - 1) / kAffineTile);
    const AffineMap *dc = reinterpret_cast<const AffineMap *>(cands);
    for_cand_frame_chunks(tiles, K, n, [&](int k0, int ck, int f0, int cf) {
        ScopedTiming timing(KIND_SVD, cx);
        OFMK_TIMED_LAUNCH(timing, svd_affine_scores_rgb8_kernel, dim3((unsigned)tiles, (unsigned)ck, (unsigned)cf), dim3(kThreads), 0, cx.s,
                          in + (size_t)f0 * a.frame_stride, dc + k0, a, reinterpret_cast<unsigned long long *>(scores) + (size_t)f0 * K + k0);
        return OFMK_OK;
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// The dense shift search (affine_phase_kernels.hiph): scores[f][k][8 py + px] = what ofmk_svd_affine_scores_rgb8 gives frame f under
// cands[k] (+) (py, px), int64 [n][K][64]; units[k][8 py + px] = ofmk_affine_units' count under that map, int64 [K][64] or NULL, added
// by the launches that hold the call's first frame only.  Both are cleared here whatever they held.  Chunks as above.
int ofmk_svd_affine_phase_scores_rgb8(const uint8_t *in, int n, int h, int w, int H, int W, const ofmk_affine *cands, int K, const double *scales,
                                      int blk, long long *scores, long long *units, void *stream, const ofmk_opts *opts) {
    if (int rc = check_search_args(opts, n, h, w, H, W, in && cands && scores, K)) return rc;
    SvdArgs sa;
    if (int rc = check_resync_scales(sa, scales, blk, true)) return rc;
    const Ctx cx = make_ctx(stream, opts);
    HIP_TRY(launch_zero(scores, (size_t)n * K * 64 * sizeof(long long), cx.s));
    if (units) HIP_TRY(launch_zero(units, (size_t)K * 64 * sizeof(long long), cx.s));
    AffinePhaseArgs a;
    a.h = h; a.w = w;
    a.oh = 8 * (H / 8); a.ow = 8 * (W / 8);
    a.rects_x = (a.ow + kPhaseRect - 1) / kPhaseRect;
    a.K = K;
    a.count_units = 0;
    a.frame_stride = (size_t)h * w * 3;
    a.scale = sa.scales[1];
    const long long rects = (long long)a.rects_x * ((a.oh + kPhaseRect - 1) / kPhaseRect);
    const AffineMap *dc = reinterpret_cast<const AffineMap *>(cands);
    unsigned long long *du = reinterpret_cast<unsigned long long *>(units);
    for_cand_frame_chunks(rects, K, n, [&](int k0, int ck, int f0, int cf) {
        ScopedTiming timing(KIND_SVD, cx);
        AffinePhaseArgs ac = a;
        ac.count_units = units && f0 == 0;                                       // once per call: the chunk with the first frame
        OFMK_TIMED_LAUNCH(timing, svd_affine_phase_scores_rgb8_kernel, dim3((unsigned)rects, (unsigned)ck, (unsigned)cf), dim3(kThreads), 0, cx.s,
                          in + (size_t)f0 * a.frame_stride, dc + k0, ac,
                          reinterpret_cast<unsigned long long *>(scores) + ((size_t)f0 * K + k0) * 64, units ? du + (size_t)k0 * 64 : du);
        return OFMK_OK;
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// The soft read-out of the counting units of the leak warped by *geom (HOST memory), unit (i, j) into position (i * (W / 8) + j) mod L;
// int64 [n][L], cleared here.  scales[1] <= 0 or no counting unit: all zeros.
int ofmk_svd_detect_soft_affine_rgb8(const uint8_t *in, int n, int h, int w, int H, int W, const ofmk_affine *geom, int L, const double *scales,
                                     int blk, long long *soft, void *stream, const ofmk_opts *opts) {
    return svd_detect_soft_mapped<AffineReadArgs, svd_soft_affine_rgb8_kernel>(in, n, h, w, H, W, geom, L, scales, blk, soft, stream, opts);
}

// ---- leaks read against their source frames (align_kernels.hiph; build extensions, not reference semantics) ----------------------
// sums[f][k][0..28] = the Gauss-Newton sums of leak frame f warped by cands[k] (DEVICE memory, [K]) against source frame f; int64
// [n][K][29], cleared here whatever it held; an out-of-range candidate leaves 29 zeros.  Chunks as ofmk_svd_affine_scores_rgb8.
int ofmk_align_sums_rgb8(const uint8_t *src, const uint8_t *leak, int n, int h, int w, int H, int W, const ofmk_affine *cands, int K,
                         long long *sums, void *stream, const ofmk_opts *opts) {
    if (int rc = check_search_args(opts, n, h, w, H, W, src && leak && cands && sums, K, kAlignMaxSide, " (the sums are int64)")) return rc;
    const Ctx cx = make_ctx(stream, opts);
    HIP_TRY(launch_zero(sums, (size_t)n * K * kAlignSums * sizeof(long long), cx.s));
    AlignArgs a;
    a.h = h; a.w = w; a.H = H; a.W = W;
    a.tiles_x = (W + kAlignTile - 1) / kAlignTile;
    a.K = K;
    a.leak_stride = (size_t)h * w * 3;
    a.src_stride = (size_t)H * W * 3;
    const long long tiles = (long long)a.tiles_x * ((H + kAlignTile - 1) / kAlignTile);
    const AffineMap *dc = reinterpret_cast<const AffineMap *>(cands);
    for_cand_frame_chunks(tiles, K, n, [&](int k0, int ck, int f0, int cf) {
        ScopedTiming timing(KIND_SVD, cx);
        OFMK_TIMED_LAUNCH(timing, align_sums_rgb8_kernel, dim3((unsigned)tiles, (unsigned)ck, (unsigned)cf), dim3(kThreads), 0, cx.s,
                          src + (size_t)f0 * a.src_stride, leak + (size_t)f0 * a.leak_stride, dc + k0, a,
                          reinterpret_cast<unsigned long long *>(sums) + ((size_t)f0 * K + k0) * kAlignSums);
        return OFMK_OK;
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// The 2x2 box of the registration pyramid: u8 [n][h / 2][w / 2][3], every byte written; an odd last row or column is dropped.
int ofmk_halve_rgb8(const uint8_t *in, int n, int h, int w, uint8_t *out, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    if (n <= 0) return fail(OFMK_E_ARG, "n must be positive%s");
    if (!in || !out) return fail(OFMK_E_ARG, "null pointer%s");
    if (int rc = check_leak_dims(h, w)) return rc;
    if (h / 2 < 8 || w / 2 < 8) return fail(OFMK_E_ARG, "both halved sides must be at least 8%s");
    const Ctx cx = make_ctx(stream, opts);
    HalveArgs a;
    a.w = w; a.Ho = h / 2; a.Wo = w / 2;
    a.in_stride = (size_t)h * w * 3;
    a.out_stride = (size_t)a.Ho * a.Wo * 3;
    for_chunks(n, kMaxChunk, [&](int f0, int cf) {
        ScopedTiming timing(KIND_SVD, cx);
        OFMK_TIMED_LAUNCH(timing, halve_rgb8_kernel, grid_2d(a.Ho * a.Wo, cf), dim3(kThreads), 0, cx.s, in + (size_t)f0 * a.in_stride,
                          out + (size_t)f0 * a.out_stride, a);
        return OFMK_OK;
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// ---- matching a leaked clip's frames to the source video's (temporal_kernels.hiph; build extensions, not reference semantics) -----
// sig[f][8 i + j] = the rounded mean luma of cell (i, j) of frame f; u8 [n][64], every byte written.  Frames in gridDim.x: no chunks.
int ofmk_signature_rgb8(const uint8_t *in, int n, int h, int w, uint8_t *sig, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    if (int rc = check_dims(n, h, w)) return rc;
    if (!in || !sig) return fail(OFMK_E_ARG, "null pointer%s");
    const Ctx cx = make_ctx(stream, opts);
    SignatureArgs a;
    a.h = h; a.w = w;
    a.frame_stride = (size_t)h * w * 3;
    ScopedTiming timing(KIND_SVD, cx);
    OFMK_TIMED_LAUNCH(timing, signature_rgb8_kernel, dim3((unsigned)n, 8u), dim3(kThreads), 0, cx.s, in, sig, a);
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// dist[i][t] = sum over the 64 bytes of |a[i][c] - b[t][c]|; int32 [m][N], every entry written.
int ofmk_signature_distances(const uint8_t *a, int m, const uint8_t *b, int N, int32_t *dist, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    if (m < 1 || N < 1) return fail(OFMK_E_ARG, "m and N must be at least 1%s");
    if ((long long)m * N >= (1LL << 40)) return fail(OFMK_E_ARG, "m * N must be < 2^40%s");
    if (!a || !b || !dist) return fail(OFMK_E_ARG, "null pointer%s");
    const Ctx cx = make_ctx(stream, opts);
    const int tiles = (m + kDistRows - 1) / kDistRows;
    ScopedTiming timing(KIND_SVD, cx);
    OFMK_TIMED_LAUNCH(timing, signature_distances_kernel, dim3((unsigned)((N + kThreads - 1) / kThreads), (unsigned)(tiles < kMaxChunk ? tiles : kMaxChunk)),
                      dim3(kThreads), 0, cx.s, a, m, b, N, dist);
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// res[i][j] = (sum e^2, contributing pixels) of leak frame i warped by *geom (HOST memory) against source lib[first[i] + j], j < span:
// ofmk_align_sums_rgb8's sums [27] and [28] of that pair; int64 [m][span][2], cleared here whatever it held.  first: DEVICE int32 [m];
// a source index outside 0..N-1 leaves (0, 0).
int ofmk_align_residuals_rgb8(const uint8_t *lib, int N, const uint8_t *leak, int m, int h, int w, int H, int W, const int32_t *first, int span,
                              const ofmk_affine *geom, long long *res, void *stream, const ofmk_opts *opts) {
    return align_window_sums<align_residuals_rgb8_kernel, 2>(lib, N, leak, m, h, w, H, W, first, span, geom, res, stream, opts);
}

// mom[i][j] = (n, sum l, sum s, sum l^2, sum s^2, sum l s) over ofmk_align_residuals_rgb8's contributing pixels, l the luma of leak frame
// i warped by *geom (HOST memory), s the luma of lib[first[i] + j]; int64 [m][span][6], cleared here whatever it held; the arguments and
// their rules are ofmk_align_residuals_rgb8's, and mom[3] + mom[4] - 2 mom[5] is its sum e^2, mom[0] its count.
int ofmk_align_moments_rgb8(const uint8_t *lib, int N, const uint8_t *leak, int m, int h, int w, int H, int W, const int32_t *first, int span,
                            const ofmk_affine *geom, long long *mom, void *stream, const ofmk_opts *opts) {
    return align_window_sums<align_moments_rgb8_kernel, kMomentSums>(lib, N, leak, m, h, w, H, W, first, span, geom, mom, stream, opts);
}

// rank[f][c] = the number of cells c' of signature f with (sig[f][c'], c') < (sig[f][c], c); u8 [n][64], every byte written.
int ofmk_signature_ranks(const uint8_t *sig, int n, uint8_t *rank, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    if (n < 1) return fail(OFMK_E_ARG, "n must be at least 1%s");
    if (!sig || !rank) return fail(OFMK_E_ARG, "null pointer%s");
    const Ctx cx = make_ctx(stream, opts);
    ScopedTiming timing(KIND_SVD, cx);
    OFMK_TIMED_LAUNCH(timing, signature_ranks_kernel, dim3((unsigned)(((long long)n + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0, cx.s,
                      sig, n, rank);
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// ---- leaks whose values changed: a tone curve fitted against the source frames (tone_kernels.hiph; build extensions) ----------------
// hist[f][c][v] = the number of pixels of frame f whose channel c equals v; int64 [n][3][256], cleared here whatever it held.
int ofmk_histograms_rgb8(const uint8_t *in, int n, int h, int w, long long *hist, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    if (n <= 0) return fail(OFMK_E_ARG, "n must be positive%s");
    if (int rc = check_leak_dims(h, w)) return rc;
    if (!in || !hist) return fail(OFMK_E_ARG, "null pointer%s");
    const Ctx cx = make_ctx(stream, opts);
    HIP_TRY(launch_zero(hist, (size_t)n * kToneBins * sizeof(long long), cx.s));
    HistArgs a;
    a.pixels = h * w;
    a.frame_stride = (size_t)h * w * 3;
    const int groups = a.pixels >> 2;
    const unsigned slices = (unsigned)(groups > kHistGroups ? (groups + kHistGroups - 1) / kHistGroups : 1);
    for_chunks(n, kMaxChunk, [&](int f0, int cf) {
        ScopedTiming timing(KIND_SVD, cx);
        OFMK_TIMED_LAUNCH(timing, histograms_rgb8_kernel, dim3(slices, (unsigned)cf), dim3(kThreads), 0, cx.s, in + (size_t)f0 * a.frame_stride,
                          reinterpret_cast<unsigned long long *>(hist) + (size_t)f0 * kToneBins, a);
        return OFMK_OK;
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// sums[f][k][c][v] = (the number of canvas pixels inside the leak where leak frame f warped by cands[k] (DEVICE memory, [K]) shows v in
// channel c, the sum of source frame f's channel c over them); int64 [n][K][3][256][2], cleared here whatever it held; an out-of-range
// candidate leaves zeros.  Chunks as ofmk_align_sums_rgb8.
int ofmk_tone_sums_rgb8(const uint8_t *src, const uint8_t *leak, int n, int h, int w, int H, int W, const ofmk_affine *cands, int K,
                        long long *sums, void *stream, const ofmk_opts *opts) {
    if (int rc = check_search_args(opts, n, h, w, H, W, src && leak && cands && sums, K, kAlignMaxSide)) return rc;
    const Ctx cx = make_ctx(stream, opts);
    HIP_TRY(launch_zero(sums, (size_t)n * K * kToneWords * sizeof(long long), cx.s));
    ToneSumsArgs a;
    a.h = h; a.w = w; a.H = H; a.W = W;
    a.tiles_x = (W + kAlignTile - 1) / kAlignTile;
    a.K = K;
    a.leak_stride = (size_t)h * w * 3;
    a.src_stride = (size_t)H * W * 3;
    const long long tiles = (long long)a.tiles_x * ((H + kAlignTile - 1) / kAlignTile);
    const AffineMap *dc = reinterpret_cast<const AffineMap *>(cands);
    for_cand_frame_chunks(tiles, K, n, [&](int k0, int ck, int f0, int cf) {
        ScopedTiming timing(KIND_SVD, cx);
        OFMK_TIMED_LAUNCH(timing, tone_sums_rgb8_kernel, dim3((unsigned)tiles, (unsigned)ck, (unsigned)cf), dim3(kThreads), 0, cx.s,
                          src + (size_t)f0 * a.src_stride, leak + (size_t)f0 * a.leak_stride, dc + k0, a,
                          reinterpret_cast<unsigned long long *>(sums) + ((size_t)f0 * K + k0) * kToneWords);
        return OFMK_OK;
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// out[f][y][x][c] = lut[c][in[f][y][x][c]]: u8 [n][h][w][3], every byte written; lut is DEVICE u8 [3][256]; out == in is allowed.
int ofmk_apply_tone_rgb8(const uint8_t *in, int n, int h, int w, const uint8_t *lut, uint8_t *out, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    if (n <= 0) return fail(OFMK_E_ARG, "n must be positive%s");
    if (int rc = check_leak_dims(h, w)) return rc;
    if (!in || !lut || !out) return fail(OFMK_E_ARG, "null pointer%s");
    const Ctx cx = make_ctx(stream, opts);
    const size_t bytes = (size_t)n * h * w * 3, steps = (bytes / 12 + kThreads - 1) / kThreads;
    const unsigned grid = (unsigned)(steps < 1 ? 1 : steps > 32768 ? 32768 : steps);      // beyond that a thread walks several groups
    ScopedTiming timing(KIND_SVD, cx);
    OFMK_TIMED_LAUNCH(timing, apply_tone_rgb8_kernel, dim3(grid), dim3(kThreads), 0, cx.s, in, out, lut, bytes);
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// ---- leaks whose colours changed: a matrix fitted against the source frames (colour_kernels.hiph; build extensions) ------------------
// sums[f][k][0..27] = the least-squares sums of source frame f against leak frame f warped by cands[k] (DEVICE memory, [K]) over the
// canvas pixels inside the leak whose warped bytes are all in 1..254; int64 [n][K][28], cleared here whatever it held; an out-of-range
// candidate leaves 28 zeros.  Chunks as ofmk_align_sums_rgb8.
int ofmk_colour_sums_rgb8(const uint8_t *src, const uint8_t *leak, int n, int h, int w, int H, int W, const ofmk_affine *cands, int K,
                          long long *sums, void *stream, const ofmk_opts *opts) {
    if (int rc = check_search_args(opts, n, h, w, H, W, src && leak && cands && sums, K, kAlignMaxSide)) return rc;
    const Ctx cx = make_ctx(stream, opts);
    HIP_TRY(launch_zero(sums, (size_t)n * K * kColourSums * sizeof(long long), cx.s));
    AlignArgs a;
    a.h = h; a.w = w; a.H = H; a.W = W;
    a.tiles_x = (W + kAlignTile - 1) / kAlignTile;
    a.K = K;
    a.leak_stride = (size_t)h * w * 3;
    a.src_stride = (size_t)H * W * 3;
    const long long tiles = (long long)a.tiles_x * ((H + kAlignTile - 1) / kAlignTile);
    const AffineMap *dc = reinterpret_cast<const AffineMap *>(cands);
    for_cand_frame_chunks(tiles, K, n, [&](int k0, int ck, int f0, int cf) {
        ScopedTiming timing(KIND_SVD, cx);
        OFMK_TIMED_LAUNCH(timing, colour_sums_rgb8_kernel, dim3((unsigned)tiles, (unsigned)ck, (unsigned)cf), dim3(kThreads), 0, cx.s,
                          src + (size_t)f0 * a.src_stride, leak + (size_t)f0 * a.leak_stride, dc + k0, a,
                          reinterpret_cast<unsigned long long *>(sums) + ((size_t)f0 * K + k0) * kColourSums);
        return OFMK_OK;
    });
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// out[c] = clip((m[c][0] in[0] + m[c][1] in[1] + m[c][2] in[2] + m[c][3] + 32768) >> 16, 0, 255) per pixel: u8 [n][h][w][3], every byte
// written; matrix is HOST int32 [3][4] in Q16, read here and passed by value; out == in is allowed.
int ofmk_apply_colour_rgb8(const uint8_t *in, int n, int h, int w, const int32_t *matrix, uint8_t *out, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    if (n <= 0) return fail(OFMK_E_ARG, "n must be positive%s");
    if (int rc = check_leak_dims(h, w)) return rc;
    if (!in || !matrix || !out) return fail(OFMK_E_ARG, "null pointer%s");
    ColourMatrix cm;
    for (int c = 0; c < 3; ++c)
        for (int j = 0; j < 4; ++j) {
            const long long v = matrix[4 * c + j], lim = j < 3 ? (1LL << 21) : (1LL << 28);     // the sum stays inside int32
            if (v < -lim || v > lim) return fail(OFMK_E_ARG, "matrix: |coefficient| <= 2^21 and |offset| <= 2^28%s");
            cm.m[c][j] = (int32_t)v;
        }
    const Ctx cx = make_ctx(stream, opts);
    const size_t bytes = (size_t)n * h * w * 3, steps = (bytes / 12 + kThreads - 1) / kThreads;
    const unsigned grid = (unsigned)(steps < 1 ? 1 : steps > 32768 ? 32768 : steps);      // beyond that a thread walks several groups
    ScopedTiming timing(KIND_SVD, cx);
    OFMK_TIMED_LAUNCH(timing, apply_colour_rgb8_kernel, dim3(grid), dim3(kThreads), 0, cx.s, in, out, cm, bytes);
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// Build extension, not reference semantics (dct_resync_kernels.hiph): scores[f][8 py + px] = sum of |soft metric| over the full 8x8
// windows of frame f at grid phase (py, px), each phase under the frame mean of ITS crop; int64 [n][64], cleared here whatever it
// held.  H, W: any values >= 8.
size_t ofmk_sync_workspace_bytes(int frames_in_flight, int H, int W) {
    if (frames_in_flight < 1 || H < 8 || W < 8 || (long long)H * W >= (1LL << 28)) return 0;
    return sync_per_frame_bytes(rgb8_leak(H, W)) * (size_t)frames_in_flight + kFixedBytes;
}

int ofmk_sync_scores_rgb8(const uint8_t *in, int n, int H, int W, double alpha, long long *scores, int chunk_frames, void *workspace,
                          size_t workspace_bytes, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    if (int rc = check_dims(n, H, W)) return rc;
    if (!in || !scores) return fail(OFMK_E_ARG, "null pointer%s");
    return sync_scores(rgb8_leak(H, W), in, n, alpha, scores, chunk_frames, workspace, workspace_bytes, stream, opts);
}

// Build extension, not reference semantics (dct_resync_kernels.hiph): the soft read-out of the blocks at grid phase (py, px) -- block
// (i, j) is the 8x8 block at pixel (py + 8i, px + 8j) -- added into position (base + i * canvas_cols + j) mod L; int64 [n][L], cleared
// here.  Masks and frame mean come from the window.  py = px = 0, canvas_cols = W / 8, base = 0 on frames with H, W multiples of
// 8: ofmk_detect_soft_rgb8, integer for integer.
int ofmk_detect_soft_window_rgb8(const uint8_t *in, int n, int H, int W, int py, int px, int canvas_cols, int base, int L, double alpha,
                                 long long *soft, int chunk_frames, void *workspace, size_t workspace_bytes, void *stream,
                                 const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    if (int rc = check_soft_args(in, n, H, W, L, soft)) return rc;
    return soft_window(rgb8_leak(H, W), in, n, py, px, canvas_cols, base, L, alpha, soft, chunk_frames, workspace, workspace_bytes, stream,
                       opts);
}

int ofmk_svd_embed_detect_rgb8(const uint8_t *in, uint8_t *out, int n, int H, int W, const uint8_t *wm, int n_wm,
                               const int32_t *wm_row, const double *scales, int blk, int L, int32_t *counts, uint8_t *bits,
                               void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    int rc = check_embed_args(in, out, n, H, W, wm, n_wm);
    if (rc) return rc;
    if ((rc = check_blk(blk))) return rc;
    if ((rc = check_detect_args(out, n, H, W, L, counts, bits))) return rc;
    SvdArgs a;
    if ((rc = make_svd_args(a, H, W, scales, false, wm, n_wm, wm_row, L, counts, bits, opts))) return rc;
    return launch_svd_rgb8(in, out, n, H, W, SVD_EMBED_VERIFY, blk, a, make_ctx(stream, opts));
}

int ofmk_embed_copies_rgb8(const uint8_t *in, uint8_t *out, int copies, int n, int H, int W, const uint8_t *wm, int n_wm,
                           const int32_t *wm_rows, double alpha, int chunk_frames, void *workspace, size_t workspace_bytes,
                           void *stream, const ofmk_opts *opts) {
    if (int rc = check_opts(opts)) return rc;
    if (int rc = check_embed_args(in, out, n, H, W, wm, n_wm)) return rc;
    const FrameFmt f = rgb8_frames(H, W);
    if (int rc = check_copies(in, out, copies, n, f.frame_bytes)) return rc;
    return embed_copies_frames(f, in, out, copies, n, wm, n_wm, wm_rows, alpha, chunk_frames, workspace, workspace_bytes, stream, opts);
}

size_t ofmk_copies_workspace_bytes(int frames_in_flight, int copies, int H, int W) {
    if (frames_in_flight < 1 || copies < 1 || copies > kMaxCopies || H < 8 || W < 8) return 0;
    return per_frame_copies_bytes(copies, H, W) * (size_t)frames_in_flight + kFixedBytes;
}

int ofmk_embed_detect_copies_rgb8(const uint8_t *in, uint8_t *out, int copies, int n, int H, int W, const uint8_t *wm, int n_wm,
                                  const int32_t *wm_rows, double alpha, int L, int32_t *counts, uint8_t *bits, int chunk_frames,
                                  void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts) {
    if (int rc = check_opts(opts)) return rc;
    if (int rc = check_embed_args(in, out, n, H, W, wm, n_wm)) return rc;
    const FrameFmt f = rgb8_frames(H, W);
    if (int rc = check_copies(in, out, copies, n, f.frame_bytes)) return rc;
    if (int rc = check_detect_args(out, n, H, W, L, counts, bits)) return rc;
    return embed_detect_copies_frames(f, in, out, copies, n, wm, n_wm, wm_rows, alpha, L, counts, bits, nullptr, chunk_frames, workspace,
                                      workspace_bytes, stream, opts);
}

// counts and bits are optional here, soft is required
int ofmk_embed_detect_copies_soft_rgb8(const uint8_t *in, uint8_t *out, int copies, int n, int H, int W, const uint8_t *wm, int n_wm,
                                       const int32_t *wm_rows, double alpha, int L, int32_t *counts, uint8_t *bits, long long *soft,
                                       int chunk_frames, void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts) {
    if (int rc = check_opts(opts)) return rc;
    if (int rc = check_embed_args(in, out, n, H, W, wm, n_wm)) return rc;
    const FrameFmt f = rgb8_frames(H, W);
    if (int rc = check_copies(in, out, copies, n, f.frame_bytes)) return rc;
    if (int rc = check_soft_args(out, n, H, W, L, soft)) return rc;
    return embed_detect_copies_frames(f, in, out, copies, n, wm, n_wm, wm_rows, alpha, L, counts, bits, soft, chunk_frames, workspace,
                                      workspace_bytes, stream, opts);
}

int ofmk_svd_embed_copies_soft_rgb8(const uint8_t *in, uint8_t *out, int copies, int n, int H, int W, const uint8_t *wm, int n_wm,
                                    const int32_t *wm_rows, const double *scales, int blk, int L, int32_t *counts, uint8_t *bits,
                                    long long *soft, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    int rc = check_embed_args(in, out, n, H, W, wm, n_wm);
    if (rc) return rc;
    if ((rc = check_copies(in, out, copies, n, (size_t)H * W * 3))) return rc;
    if ((rc = check_blk(blk))) return rc;
    if ((rc = check_soft_args(out, n, H, W, L, soft))) return rc;
    SvdArgs a;
    if ((rc = make_svd_args(a, H, W, scales, false, wm, n_wm, nullptr, L, counts, bits, opts))) return rc;
    const int mode = counts || bits ? SVD_EMBED_VERIFY : SVD_EMBED;
    const Ctx cx = make_ctx(stream, opts);
    return svd_copies_soft(out, (size_t)H * W * 3, copies, n, H, W, blk, L, wm_rows, a, soft, cx,
        [&](const SvdArgs &b, long long *sf) { return launch_svd_copies_rgb8(in, out, copies, n, H, W, wm_rows, b, cx, sf); },
        [&](uint8_t *out_q, const SvdArgs &b) { return launch_svd_rgb8(in, out_q, n, H, W, mode, 8, b, cx); },
        [&](uint8_t *out_q, const SvdArgs &b) { return launch_svd_rgb8(out_q, nullptr, n, H, W, SVD_DETECT_SOFT, 8, b, cx); });
}

int ofmk_svd_embed_copies_rgb8(const uint8_t *in, uint8_t *out, int copies, int n, int H, int W, const uint8_t *wm, int n_wm,
                               const int32_t *wm_rows, const double *scales, int blk, int L, int32_t *counts, uint8_t *bits,
                               void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    int rc = check_embed_args(in, out, n, H, W, wm, n_wm);
    if (rc) return rc;
    if ((rc = check_copies(in, out, copies, n, (size_t)H * W * 3))) return rc;
    if ((rc = check_blk(blk))) return rc;
    SvdArgs a;
    if ((rc = make_svd_args(a, H, W, scales, false, wm, n_wm, nullptr, L, counts, bits, opts))) return rc;
    const int mode = counts || bits ? SVD_EMBED_VERIFY : SVD_EMBED;
    const Ctx cx = make_ctx(stream, opts);
    if (blk == 4) return launch_svd_copies_rgb8(in, out, copies, n, H, W, wm_rows, a, cx);
    return launch_svd8_copies(out, (size_t)H * W * 3, copies, n, H, W, wm_rows, a,
                              [&](uint8_t *out_q, const SvdArgs &b) { return launch_svd_rgb8(in, out_q, n, H, W, mode, 8, b, cx); });
}

int ofmk_svd_encode_yuv32f(float *yuv, int n, int H, int W, const uint8_t *wm, int n_wm, const int32_t *wm_row,
                           const double *scales, int blk, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    int rc = check_embed_args(yuv, yuv, n, H, W, wm, n_wm);
    if (rc) return rc;
    if ((rc = check_blk(blk))) return rc;
    if (n > kMaxChunk) return fail(OFMK_E_ARG, "too many frames%s");
    SvdArgs a;
    if ((rc = make_svd_args(a, H, W, scales, false, wm, n_wm, wm_row, 1, nullptr, nullptr, nullptr))) return rc;
    const Ctx cx = make_ctx(stream, opts);
    if (blk == 8) {
        const Geom8 g8 = make_geom8(H, W);
        if (g8.ntile > 0) {                               // an event pair is reserved only for a launch that happens
            ScopedTiming timing(KIND_SVD, cx);
            OFMK_TIMED_LAUNCH(timing, (svd8_yuv32f_kernel<SVD_EMBED>), grid_2d(g8.ntile, n), dim3(kThreads), 0, cx.s, yuv, g8,
                              to_args8(a, (int)((long long)H * W / 256)));
        }
        HIP_TRY(hipGetLastError());
        return OFMK_OK;
    }
    const Geom g = svd_geom(H, W);
    ScopedTiming timing(KIND_SVD, cx);                    // the plugin path's launches are timed like every other
    OFMK_TIMED_LAUNCH(timing, (svd_yuv32f_kernel<SVD_EMBED>), grid_2d(g.nblk, n), dim3(kThreads), 0, cx.s, yuv, g, a);
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

int ofmk_svd_decode_yuv32f(const float *yuv, int n, int H, int W, const double *scales, int blk, uint8_t *bits, void *stream,
                           const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    int rc = check_dims(n, H, W);
    if (rc) return rc;
    if ((rc = check_blk(blk))) return rc;
    if (!yuv || !bits) return fail(OFMK_E_ARG, "null pointer%s");
    if (n > kMaxChunk) return fail(OFMK_E_ARG, "too many frames%s");
    SvdArgs a;
    if ((rc = make_svd_args(a, H, W, scales, true, nullptr, 0, nullptr, 1, nullptr, bits, nullptr))) return rc;
    const Ctx cx = make_ctx(stream, opts);
    hipStream_t s = cx.s;
    if (blk == 8) {                                       // bits: [n][H*W/256] (dwt_dct_svd_decoder.py:14)
        const Geom8 g8 = make_geom8(H, W);
        const Svd8Args a8 = to_args8(a, (int)((long long)H * W / 256));
        if (a8.N8 > g8.ntile || !(a.scales[1] > 0.f)) HIP_TRY(launch_zero(bits, (size_t)n * a8.N8, s));
        if (!(a.scales[1] > 0.f) || g8.ntile == 0) return OFMK_OK;
        ScopedTiming timing(KIND_SVD, cx);
        OFMK_TIMED_LAUNCH(timing, (svd8_yuv32f_kernel<SVD_DETECT>), grid_2d(g8.ntile, n), dim3(kThreads), 0, s, const_cast<float *>(yuv), g8, a8);
        HIP_TRY(hipGetLastError());
        return OFMK_OK;
    }
    const Geom g = svd_geom(H, W);
    if (a.N > g.nblk || !(a.scales[1] > 0.f)) HIP_TRY(launch_zero(bits, (size_t)n * a.N, s));
    if (!(a.scales[1] > 0.f)) return OFMK_OK;
    ScopedTiming timing(KIND_SVD, cx);
    OFMK_TIMED_LAUNCH(timing, (svd_yuv32f_kernel<SVD_DETECT>), grid_2d(g.nblk, n), dim3(kThreads), 0, s, const_cast<float *>(yuv), g, a);
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

int ofmk_payloads_from_counts(const int32_t *counts, int n, int L, int n_bits, const int32_t *perm, uint8_t *payload,
                              void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    if (!counts || !perm || !payload) return fail(OFMK_E_ARG, "null pointer%s");
    if (n < 1 || L < 1 || n_bits < 0) return fail(OFMK_E_ARG, "bad sizes%s");
    return launch_payloads(counts, n, L, n_bits, perm, payload, static_cast<hipStream_t>(stream));
}

int ofmk_svd_count_tiles(int H, int W, int blk) {
    if (H < 8 || W < 8 || check_blk(blk)) return -1;
    return svd_count_tiles(H, W, blk);
}

int ofmk_payloads_from_partial_counts(const int32_t *partials, int tiles, int n, int L, int n_bits, const int32_t *perm,
                                      uint8_t *payload, int32_t *counts, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    if (!partials || (!payload && !counts) || (payload && !perm)) return fail(OFMK_E_ARG, "null pointer%s");
    if (n < 1 || L < 1 || n_bits < 0 || tiles < 0) return fail(OFMK_E_ARG, "bad sizes%s");
    if (L > kHistMax) return fail(OFMK_E_ARG, "partial counts need L <= 2048%s");
    if ((long long)tiles * L >= (1LL << 31)) return fail(OFMK_E_ARG, "tiles * L too large%s");
    hipLaunchKernelGGL(degenerate_partial_kernel, dim3((unsigned)n), dim3(kThreads), 0, static_cast<hipStream_t>(stream), partials, tiles, L,
                       n_bits, perm, payload, counts);
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// ---- planar YUV 4:2:0 entry points ------------------------------------------------------
int ofmk_embed_yuv420(const uint8_t *in, uint8_t *out, int layout, int n, int H, int W, const uint8_t *wm, int n_wm,
                      const int32_t *wm_row, double alpha, int chunk_frames, void *workspace, size_t workspace_bytes,
                      void *stream, const ofmk_opts *opts) {
    if (int rc = check_opts(opts)) return rc;
    if (int rc = check_embed_args(in, out, n, H, W, wm, n_wm)) return rc;
    if (int rc = check_planar(layout, H, W, in, out)) return rc;
    return embed_frames(yuv420_frames(layout, H, W), in, out, n, wm, n_wm, wm_row, alpha, chunk_frames, workspace, workspace_bytes, stream,
                        opts);
}

int ofmk_detect_yuv420(const uint8_t *in, int layout, int n, int H, int W, int L, double alpha, int32_t *counts, uint8_t *bits,
                       int chunk_frames, void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts) {
    if (int rc = check_opts(opts)) return rc;
    if (int rc = check_detect_args(in, n, H, W, L, counts, bits)) return rc;
    if (int rc = check_planar(layout, H, W, in, nullptr)) return rc;
    return detect_frames(yuv420_frames(layout, H, W), in, n, L, alpha, counts, bits, nullptr, chunk_frames, workspace, workspace_bytes,
                         stream, opts);
}

// The DCT codec's soft metric (ofmk_detect_soft_rgb8) for planar callers: the planar analysis, then the same finalize.
int ofmk_detect_soft_yuv420(const uint8_t *in, int layout, int n, int H, int W, int L, double alpha, long long *soft, int chunk_frames,
                            void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts) {
    if (int rc = check_opts(opts)) return rc;
    if (int rc = check_soft_args(in, n, H, W, L, soft)) return rc;
    if (int rc = check_planar(layout, H, W, in, nullptr)) return rc;
    return detect_frames(yuv420_frames(layout, H, W), in, n, L, alpha, nullptr, nullptr, soft, chunk_frames, workspace, workspace_bytes,
                         stream, opts);
}

int ofmk_embed_detect_yuv420(const uint8_t *in, uint8_t *out, int layout, int n, int H, int W, const uint8_t *wm, int n_wm,
                             const int32_t *wm_row, double alpha, int L, int32_t *counts, uint8_t *bits, int chunk_frames,
                             void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts) {
    if (int rc = check_opts(opts)) return rc;
    if (int rc = check_embed_args(in, out, n, H, W, wm, n_wm)) return rc;
    if (int rc = check_planar(layout, H, W, in, out)) return rc;
    if (int rc = check_detect_args(out, n, H, W, L, counts, bits)) return rc;
    return embed_detect_frames(yuv420_frames(layout, H, W), in, out, n, wm, n_wm, wm_row, alpha, L, counts, bits, chunk_frames, workspace,
                               workspace_bytes, stream, opts);
}

// ---- DwtDctSvd codec on planar YUV 4:2:0: the rgb8 SVD calls' conventions, the yuv420 calls' layout ----------------------------
int ofmk_svd_embed_yuv420(const uint8_t *in, uint8_t *out, int layout, int n, int H, int W, const uint8_t *wm, int n_wm,
                          const int32_t *wm_row, const double *scales, int blk, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    int rc = check_embed_args(in, out, n, H, W, wm, n_wm);
    if (rc) return rc;
    if ((rc = check_blk(blk))) return rc;
    if ((rc = check_planar(layout, H, W, in, out))) return rc;
    SvdArgs a;
    if ((rc = make_svd_args(a, H, W, scales, false, wm, n_wm, wm_row, 1, nullptr, nullptr, nullptr))) return rc;
    return launch_svd_yuv420(in, out, layout, n, H, W, SVD_EMBED, blk, a, make_ctx(stream, opts));
}

// scales[1] <= 0: zeroed counts / bits, as ofmk_svd_detect_rgb8
int ofmk_svd_detect_yuv420(const uint8_t *in, int layout, int n, int H, int W, int L, const double *scales, int blk,
                           int32_t *counts, uint8_t *bits, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    int rc = check_detect_args(in, n, H, W, L, counts, bits);
    if (rc) return rc;
    if ((rc = check_blk(blk))) return rc;
    if ((rc = check_planar(layout, H, W, in, nullptr))) return rc;
    SvdArgs a;
    if ((rc = make_svd_args(a, H, W, scales, true, nullptr, 0, nullptr, L, counts, bits, opts))) return rc;
    if (!(a.scales[1] > 0.f)) return zero_svd_readout(n, H, W, blk, a, static_cast<hipStream_t>(stream));
    return launch_svd_yuv420(in, nullptr, layout, n, H, W, SVD_DETECT, blk, a, make_ctx(stream, opts));
}

// == ofmk_svd_detect_soft_rgb8(ofmk_yuv420_to_rgb8(in)), integer for integer (the same loads and LL band as the hard read-out)
int ofmk_svd_detect_soft_yuv420(const uint8_t *in, int layout, int n, int H, int W, int L, const double *scales, int blk,
                                long long *soft, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    int rc = check_soft_args(in, n, H, W, L, soft);
    if (rc) return rc;
    if ((rc = check_blk(blk))) return rc;
    if ((rc = check_planar(layout, H, W, in, nullptr))) return rc;
    return svd_detect_soft(n, H, W, L, scales, soft, stream, [&](const SvdArgs &a) {
        return launch_svd_yuv420(in, nullptr, layout, n, H, W, SVD_DETECT_SOFT, blk, a, make_ctx(stream, opts));
    });
}

int ofmk_svd_embed_detect_yuv420(const uint8_t *in, uint8_t *out, int layout, int n, int H, int W, const uint8_t *wm, int n_wm,
                                 const int32_t *wm_row, const double *scales, int blk, int L, int32_t *counts, uint8_t *bits,
                                 void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    int rc = check_embed_args(in, out, n, H, W, wm, n_wm);
    if (rc) return rc;
    if ((rc = check_blk(blk))) return rc;
    if ((rc = check_detect_args(out, n, H, W, L, counts, bits))) return rc;
    if ((rc = check_planar(layout, H, W, in, out))) return rc;
    SvdArgs a;
    if ((rc = make_svd_args(a, H, W, scales, false, wm, n_wm, wm_row, L, counts, bits, opts))) return rc;
    return launch_svd_yuv420(in, out, layout, n, H, W, SVD_EMBED_VERIFY, blk, a, make_ctx(stream, opts));
}

// ---- C marked copies on planar YUV 4:2:0 (planar_copies_kernels.hiph) ----------------------------------------------------------
int ofmk_embed_copies_yuv420(const uint8_t *in, uint8_t *out, int layout, int copies, int n, int H, int W, const uint8_t *wm, int n_wm,
                             const int32_t *wm_rows, double alpha, int chunk_frames, void *workspace, size_t workspace_bytes,
                             void *stream, const ofmk_opts *opts) {
    if (int rc = check_opts(opts)) return rc;
    if (int rc = check_embed_args(in, out, n, H, W, wm, n_wm)) return rc;
    if (int rc = check_planar(layout, H, W, in, out)) return rc;
    const FrameFmt f = yuv420_frames(layout, H, W);
    if (int rc = check_copies(in, out, copies, n, f.frame_bytes)) return rc;
    return embed_copies_frames(f, in, out, copies, n, wm, n_wm, wm_rows, alpha, chunk_frames, workspace, workspace_bytes, stream, opts);
}

int ofmk_embed_detect_copies_yuv420(const uint8_t *in, uint8_t *out, int layout, int copies, int n, int H, int W, const uint8_t *wm,
                                    int n_wm, const int32_t *wm_rows, double alpha, int L, int32_t *counts, uint8_t *bits,
                                    int chunk_frames, void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts) {
    if (int rc = check_opts(opts)) return rc;
    if (int rc = check_embed_args(in, out, n, H, W, wm, n_wm)) return rc;
    if (int rc = check_planar(layout, H, W, in, out)) return rc;
    const FrameFmt f = yuv420_frames(layout, H, W);
    if (int rc = check_copies(in, out, copies, n, f.frame_bytes)) return rc;
    if (int rc = check_detect_args(out, n, H, W, L, counts, bits)) return rc;
    return embed_detect_copies_frames(f, in, out, copies, n, wm, n_wm, wm_rows, alpha, L, counts, bits, nullptr, chunk_frames, workspace,
                                      workspace_bytes, stream, opts);
}

int ofmk_embed_detect_copies_soft_yuv420(const uint8_t *in, uint8_t *out, int layout, int copies, int n, int H, int W, const uint8_t *wm,
                                         int n_wm, const int32_t *wm_rows, double alpha, int L, int32_t *counts, uint8_t *bits,
                                         long long *soft, int chunk_frames, void *workspace, size_t workspace_bytes, void *stream,
                                         const ofmk_opts *opts) {
    if (int rc = check_opts(opts)) return rc;
    if (int rc = check_embed_args(in, out, n, H, W, wm, n_wm)) return rc;
    if (int rc = check_planar(layout, H, W, in, out)) return rc;
    const FrameFmt f = yuv420_frames(layout, H, W);
    if (int rc = check_copies(in, out, copies, n, f.frame_bytes)) return rc;
    if (int rc = check_soft_args(out, n, H, W, L, soft)) return rc;
    return embed_detect_copies_frames(f, in, out, copies, n, wm, n_wm, wm_rows, alpha, L, counts, bits, soft, chunk_frames, workspace,
                                      workspace_bytes, stream, opts);
}

int ofmk_svd_embed_copies_yuv420(const uint8_t *in, uint8_t *out, int layout, int copies, int n, int H, int W, const uint8_t *wm,
                                 int n_wm, const int32_t *wm_rows, const double *scales, int blk, int L, int32_t *counts,
                                 uint8_t *bits, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    int rc = check_embed_args(in, out, n, H, W, wm, n_wm);
    if (rc) return rc;
    if ((rc = check_blk(blk))) return rc;
    if ((rc = check_planar(layout, H, W, in, out))) return rc;
    const size_t fs = (size_t)H * W * 3 / 2;
    if ((rc = check_copies(in, out, copies, n, fs))) return rc;
    SvdArgs a;
    if ((rc = make_svd_args(a, H, W, scales, false, wm, n_wm, nullptr, L, counts, bits, opts))) return rc;
    const Ctx cx = make_ctx(stream, opts);
    if (blk == 4) return launch_svd_copies_yuv420(in, out, layout, copies, n, H, W, wm_rows, a, cx);
    const int mode = counts || bits ? SVD_EMBED_VERIFY : SVD_EMBED;         // per copy: the tiles, then the fringe's 4:2:0 round trip
    return launch_svd8_copies(out, fs, copies, n, H, W, wm_rows, a,
                              [&](uint8_t *out_q, const SvdArgs &b) { return launch_svd_yuv420(in, out_q, layout, n, H, W, mode, 8, b, cx); });
}

int ofmk_svd_embed_copies_soft_yuv420(const uint8_t *in, uint8_t *out, int layout, int copies, int n, int H, int W, const uint8_t *wm,
                                      int n_wm, const int32_t *wm_rows, const double *scales, int blk, int L, int32_t *counts,
                                      uint8_t *bits, long long *soft, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    int rc = check_embed_args(in, out, n, H, W, wm, n_wm);
    if (rc) return rc;
    if ((rc = check_blk(blk))) return rc;
    if ((rc = check_planar(layout, H, W, in, out))) return rc;
    const size_t fs = (size_t)H * W * 3 / 2;
    if ((rc = check_copies(in, out, copies, n, fs))) return rc;
    if ((rc = check_soft_args(out, n, H, W, L, soft))) return rc;
    SvdArgs a;
    if ((rc = make_svd_args(a, H, W, scales, false, wm, n_wm, nullptr, L, counts, bits, opts))) return rc;
    const int mode = counts || bits ? SVD_EMBED_VERIFY : SVD_EMBED;
    const Ctx cx = make_ctx(stream, opts);
    return svd_copies_soft(out, fs, copies, n, H, W, blk, L, wm_rows, a, soft, cx,
        [&](const SvdArgs &b, long long *sf) { return launch_svd_copies_yuv420(in, out, layout, copies, n, H, W, wm_rows, b, cx, sf); },
        [&](uint8_t *out_q, const SvdArgs &b) { return launch_svd_yuv420(in, out_q, layout, n, H, W, mode, 8, b, cx); },
        [&](uint8_t *out_q, const SvdArgs &b) { return launch_svd_yuv420(out_q, nullptr, layout, n, H, W, SVD_DETECT_SOFT, 8, b, cx); });
}

int ofmk_yuv420_to_rgb8(const uint8_t *yuv, uint8_t *rgb, int layout, int n, int H, int W, void *stream, const ofmk_opts *opts) {
    return convert_yuv420(const_cast<uint8_t *>(yuv), rgb, true, layout, n, H, W, stream, opts);
}

int ofmk_rgb8_to_yuv420(const uint8_t *rgb, uint8_t *yuv, int layout, int n, int H, int W, void *stream, const ofmk_opts *opts) {
    return convert_yuv420(yuv, const_cast<uint8_t *>(rgb), false, layout, n, H, W, stream, opts);
}

// ---- block-grid resync on 4:2:0 planes (planar_resync_kernels.hiph; build extension, not reference semantics) -------------------
// scores[f][8 py + px], even py and px with a full unit: the sum of |unit metric| of ofmk_svd_detect_soft_yuv420 (blk 4) on the
// frame's sub-planes for the pixel window [py : py + 8r, px : px + 8c]; every other entry 0 (an odd crop offset does not exist on
// 4:2:0 planes).  int64 [n][64], cleared here whatever it held.  H, W: even, >= 8; no alignment asked of `in`.
int ofmk_svd_sync_scores_yuv420(const uint8_t *in, int layout, int n, int H, int W, const double *scales, int blk, long long *scores,
                                void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    if (int rc = check_dims(n, H, W)) return rc;
    if (!in || !scores) return fail(OFMK_E_ARG, "null pointer%s");
    return svd_sync_scores(yuv420_leak(layout, H, W), in, n, scales, blk, scores, stream, opts);
}

// The soft read-out of the units at the even phase (py, px), read through the frame's own pitch, added into position
// (base + i * canvas_cols + j) mod L; int64 [n][L], cleared here.  py = px = 0, canvas_cols = W / 8, base = 0 on frames with H, W
// multiples of 8: ofmk_svd_detect_soft_yuv420 (blk 4), integer for integer.  scales[1] <= 0: all zeros, as that call.
int ofmk_svd_detect_soft_window_yuv420(const uint8_t *in, int layout, int n, int H, int W, int py, int px, int canvas_cols, int base, int L,
                                       const double *scales, int blk, long long *soft, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    if (int rc = check_soft_args(in, n, H, W, L, soft)) return rc;
    return svd_soft_window(yuv420_leak(layout, H, W), in, n, py, px, canvas_cols, base, L, scales, blk, soft, stream, opts);
}

// The DCT codec's planar search: scratch for `frames_in_flight` frames (12 bytes per EVEN pixel origin and 16 sums per frame).
size_t ofmk_sync_workspace_bytes_yuv420(int frames_in_flight, int H, int W) {
    if (frames_in_flight < 1 || H < 8 || W < 8 || H % 2 || W % 2 || (long long)H * W >= (1LL << 28)) return 0;
    return sync_per_frame_bytes(yuv420_leak(OFMK_YUV_I420, H, W)) * (size_t)frames_in_flight + kFixedBytes;      // the same for NV12
}

// scores[f][8 py + px], even py and px with a full block: the sum of |block metric| of ofmk_detect_soft_yuv420 on the frame's
// sub-planes for the pixel window [py : py + 8r, px : px + 8c], masks and frame mean from that sub-frame; every other entry 0.
int ofmk_sync_scores_yuv420(const uint8_t *in, int layout, int n, int H, int W, double alpha, long long *scores, int chunk_frames,
                            void *workspace, size_t workspace_bytes, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    if (int rc = check_dims(n, H, W)) return rc;
    if (!in || !scores) return fail(OFMK_E_ARG, "null pointer%s");
    return sync_scores(yuv420_leak(layout, H, W), in, n, alpha, scores, chunk_frames, workspace, workspace_bytes, stream, opts);
}

// The soft read-out of the blocks at the even phase (py, px), with canvas positions; masks and frame mean come from the window.
// py = px = 0, canvas_cols = W / 8, base = 0 on frames with H, W multiples of 8: ofmk_detect_soft_yuv420, integer for integer.
int ofmk_detect_soft_window_yuv420(const uint8_t *in, int layout, int n, int H, int W, int py, int px, int canvas_cols, int base, int L,
                                   double alpha, long long *soft, int chunk_frames, void *workspace, size_t workspace_bytes, void *stream,
                                   const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    if (int rc = check_soft_args(in, n, H, W, L, soft)) return rc;
    return soft_window(yuv420_leak(layout, H, W), in, n, py, px, canvas_cols, base, L, alpha, soft, chunk_frames, workspace, workspace_bytes,
                       stream, opts);
}

int ofmk_probe_xcc(int32_t *xcc_of_workgroup, int n_workgroups, void *stream, const ofmk_opts *opts) {
    if (int orc = check_opts(opts)) return orc;
    if (!xcc_of_workgroup || n_workgroups < 1 || n_workgroups > (1 << 20)) return fail(OFMK_E_ARG, "probe needs an output array and 1..2^20 workgroups%s");
    hipLaunchKernelGGL(probe_xcc_kernel, dim3((unsigned)n_workgroups), dim3(64), 0, static_cast<hipStream_t>(stream), xcc_of_workgroup, n_workgroups);
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

// ---- timing objects (caller-owned; see the header) ------------------------------------------------
int ofmk_timing_create(int max_launches, unsigned kind_mask, ofmk_timing **out) {
    if (!out) return fail(OFMK_E_ARG, "null output%s");
    *out = nullptr;
    if (max_launches < 1) return fail(OFMK_E_ARG, "max_launches must be positive%s");
    ofmk_timing *t = new ofmk_timing;
    t->rec = new TimingRec[max_launches];
    t->cap = max_launches;
    t->used.store(0);
    t->mask = kind_mask ? kind_mask : 0xFFFFFFFFu;
    for (int i = 0; i < max_launches; ++i) { t->rec[i].a = nullptr; t->rec[i].b = nullptr; t->rec[i].kind = -1; }
    for (int i = 0; i < max_launches; ++i) {
        hipError_t e = hipEventCreate(&t->rec[i].a);
        if (e == hipSuccess) e = hipEventCreate(&t->rec[i].b);
        if (e != hipSuccess) {
            ofmk_timing_destroy(t);                 // destroys whichever events exist (the others are null)
            return fail(OFMK_E_HIP, "hipEventCreate: %s", hipGetErrorString(e));
        }
    }
    *out = t;
    return OFMK_OK;
}

int ofmk_timing_collect(ofmk_timing *t, double *ms_by_kind, int *launches_by_kind) {
    if (!t || !ms_by_kind || !launches_by_kind) return fail(OFMK_E_ARG, "null pointer%s");
    for (int k = 0; k < KIND_COUNT; ++k) { ms_by_kind[k] = 0.0; launches_by_kind[k] = 0; }
    const int taken = t->used.load();
    const int used = taken < t->cap ? taken : t->cap;
    int rc = OFMK_OK;
    for (int i = 0; i < used; ++i) {
        // a pair whose launch failed after it was reserved was never recorded: skip it, do not poison the pool
        float ms = 0.f;
        hipError_t e = hipEventSynchronize(t->rec[i].b);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, t->rec[i].a, t->rec[i].b);
        if (e == hipSuccess && t->rec[i].kind >= 0 && t->rec[i].kind < KIND_COUNT) {
            ms_by_kind[t->rec[i].kind] += ms;
            launches_by_kind[t->rec[i].kind] += 1;
        } else if (e != hipSuccess && e != hipErrorInvalidHandle && e != hipErrorInvalidResourceHandle && e != hipErrorNotReady) {
            rc = fail(OFMK_E_HIP, "timing collect: %s", hipGetErrorString(e));
        }
        if (e != hipSuccess) (void)hipGetLastError();
        t->rec[i].kind = -1;
    }
    t->used.store(0);
    if (rc) return rc;
    return OFMK_OK;
}

int ofmk_timing_durations(ofmk_timing *t, float *ms_per_launch, int *kind_per_launch, int cap) {
    if (!t || !ms_per_launch || cap < 0) return fail(OFMK_E_ARG, "null pointer%s");
    const int taken = t->used.load();
    const int used = taken < t->cap ? taken : t->cap;
    int n = 0;
    for (int i = 0; i < used && n < cap; ++i) {
        float ms = 0.f;
        hipError_t e = hipEventSynchronize(t->rec[i].b);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, t->rec[i].a, t->rec[i].b);
        if (e != hipSuccess) { (void)hipGetLastError(); continue; }      // a pair whose launch failed was never recorded
        ms_per_launch[n] = ms;
        if (kind_per_launch) kind_per_launch[n] = t->rec[i].kind;
        ++n;
    }
    return n;
}

void ofmk_timing_destroy(ofmk_timing *t) {
    if (!t) return;
    for (int i = 0; i < t->cap; ++i) {
        if (t->rec[i].a) (void)hipEventDestroy(t->rec[i].a);
        if (t->rec[i].b) (void)hipEventDestroy(t->rec[i].b);
    }
    delete[] t->rec;
    delete t;
}

// ---- streaming probes: the device's achievable HBM rates, measured in the same run as the kernels ----
int ofmk_hbm_copy(const void *src, void *dst, size_t bytes, void *stream) {
    if (!src || !dst || bytes % 16 || (uintptr_t)src % 16 || (uintptr_t)dst % 16)
        return fail(OFMK_E_ARG, "copy needs 16-byte aligned pointers and size%s");
    const size_t n16 = bytes / 16;
    if (n16 == 0) return OFMK_OK;
    hipLaunchKernelGGL(copy16_kernel, dim3((unsigned)((n16 + kCopyPerWg - 1) / kCopyPerWg)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), static_cast<const uint4 *>(src), static_cast<uint4 *>(dst), n16);
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

int ofmk_hbm_read(const void *src, size_t bytes, void *sink, void *stream) {
    if (!src || !sink || bytes % 16 || (uintptr_t)src % 16 || (uintptr_t)sink % 4)
        return fail(OFMK_E_ARG, "read probe needs a 16-byte aligned source and size, and a 4-byte sink%s");
    const size_t n16 = bytes / 16;
    if (n16 == 0) return OFMK_OK;
    hipLaunchKernelGGL(read16_kernel, dim3((unsigned)((n16 + kReadPerWg - 1) / kReadPerWg)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), static_cast<const uint4 *>(src), n16, static_cast<uint32_t *>(sink));
    HIP_TRY(hipGetLastError());
    return OFMK_OK;
}

}  // extern "C"
