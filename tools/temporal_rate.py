"""Reading a leaked CLIP (build extension): the three device calls that match its frames to the source video's, and the whole recipe.
The workload: a 300-frame 1080p dissolve (key frames every 8 frames, offmark.synthetic), DwtDctSvd-marked on the device in segments of
8 frames; the leak is 48 of its frames from frame 100 on with every sixth dropped, rotated by 1 degree about the centre (float64
bilinear, on the device) and cropped off-centre to 1001 x 1801 (tools/affine_phase_rate.py's crop).  The library is the unmarked video.
  (a) signatures of the whole library against the same bytes from torch integer passes (asserted identical), and as a fraction of the
      read rate ofmk_hbm_read reaches in this run (bench.py --full's probe, same repetitions)
  (b) signature_distances (48 x 300) against torch.cdist(p=1) on float32 copies made outside the timing (exact at these magnitudes;
      asserted identical)
  (c) align_residuals at span 7 over the 48 leak frames against index_select + align_sums per offset (asserted identical)
  (d) the whole read_leak_clip (host time, synchronisations and float64 solves included), with what it found.
The routes of a comparison alternate call by call in one process; per row the median of --reps calls after --warmup and the spread
(min..max of the repetitions).  A verdict is only given beyond the spread: one route's slowest call beats the other's fastest.
usage: python tools/temporal_rate.py [--frames 300] [--leak 48] [--reps 30] [--warmup 2] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-fingerprinting_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from affine_phase_rate import COLS, ROWS  # noqa: E402
from align_rate import alternate_wall, row, verdict  # noqa: E402
from copies_verify_rate import alternate, source_sha16  # noqa: E402
from offmark import _hip, resync, temporal  # noqa: E402
from offmark.engine import DctEngine  # noqa: E402
from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder  # noqa: E402
from offmark.fingerprint import payload_for_segment  # noqa: E402
from offmark.generator.shuffler import Shuffler  # noqa: E402
from offmark.synthetic import synthetic_frames  # noqa: E402

PER, L, ANGLE, SPAN, FIRST_FRAME = 8, 8, 1.0, 7, 100


def dissolve(n, H, W, seed):
    """u8 [n, H, W, 3] on the device: frame t = ((8 - t % 8) K[t // 8] + (t % 8) K[t // 8 + 1] + 4) // 8 over synthetic key frames."""
    K = synthetic_frames(n // PER + 2, H, W, seed=seed).to(torch.int16)
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=K.device)
    for t in range(n):
        out[t] = (((PER - t % PER) * K[t // PER] + (t % PER) * K[t // PER + 1] + 4) // PER).to(torch.uint8)
    return out


def rotate(frames, angle_deg):
    """tools/affine_rate.py's rotation on the device: pixel p samples the frame at R(angle) (p - c) + c, clamped; float64 bilinear."""
    n, H, W = frames.shape[:3]
    a = float(np.deg2rad(angle_deg))
    dev = frames.device
    dy = torch.arange(H, dtype=torch.float64, device=dev)[:, None] - (H - 1) / 2.0
    dx = torch.arange(W, dtype=torch.float64, device=dev)[None, :] - (W - 1) / 2.0
    sy = (np.cos(a) * dy - np.sin(a) * dx + (H - 1) / 2.0).clamp(0.0, H - 1.0)
    sx = (np.sin(a) * dy + np.cos(a) * dx + (W - 1) / 2.0).clamp(0.0, W - 1.0)
    y0, x0 = sy.floor().long(), sx.floor().long()
    y1, x1 = (y0 + 1).clamp(max=H - 1), (x0 + 1).clamp(max=W - 1)
    fy, fx = (sy - y0)[:, :, None], (sx - x0)[:, :, None]
    out = torch.empty_like(frames)
    for k in range(n):
        p = frames[k].to(torch.float64)
        top = (1 - fx) * p[y0, x0] + fx * p[y0, x1]
        bot = (1 - fx) * p[y1, x0] + fx * p[y1, x1]
        out[k] = ((1 - fy) * top + fy * bot).round().clamp(0, 255).to(torch.uint8)
    return out


def torch_signatures(frames, chunk=30):
    """The signatures from torch integer passes: uint8 [n, 64]."""
    n, H, W = frames.shape[:3]
    out = torch.empty((n, 64), dtype=torch.uint8, device=frames.device)
    for f0 in range(0, n, chunk):
        p = frames[f0:f0 + chunk].to(torch.int32)
        Y = (p[..., 0] + 2 * p[..., 1] + p[..., 2] + 2) >> 2
        for i in range(8):
            for j in range(8):
                cell = Y[:, (i * H) >> 3:((i + 1) * H) >> 3, (j * W) >> 3:((j + 1) * W) >> 3]
                area = cell.shape[1] * cell.shape[2]
                out[f0:f0 + chunk, 8 * i + j] = ((2 * cell.sum(dim=(1, 2)) + area) // (2 * area)).to(torch.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--leak", type=int, default=48)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, m, H, W = args.frames, args.leak, 1080, 1920
    torch.cuda.set_device(0)
    eng = DctEngine()
    dev = eng.device
    dec = DwtDctSvdDecoder()
    library = dissolve(N, H, W, 2000)
    segments = (N + PER - 1) // PER
    chosen = [(s * 7 + 3) % 5 % 2 for s in range(segments)]
    wm = np.stack([Shuffler(key=0).generate_wm(payload_for_segment(s + 1, chosen[s]), (H * W // 64,)) for s in range(segments)]).astype(np.uint8)
    kept = [t for t in range(FIRST_FRAME, N) if t % 6 != 4][:m]
    assert len(kept) == m and kept[-1] + SPAN < N
    clip = library.index_select(0, torch.tensor(kept, device=dev))
    marked = eng.svd_embed(clip, wm, wm_row=torch.tensor([t // PER for t in kept], dtype=torch.int32, device=dev))
    leak = rotate(marked, ANGLE)[:, ROWS[0]:ROWS[1], COLS[0]:COLS[1]].contiguous()
    del marked, clip
    h, w = int(leak.shape[1]), int(leak.shape[2])
    cands = {s: [payload_for_segment(s + 1, c) for c in range(2)] for s in range(segments)}

    lines = [f"# tools/temporal_rate.py: library = a {N}-frame {H}x{W} dissolve (key frames every {PER}); leak = {m} of its frames from frame "
             f"{FIRST_FRAME} on with every sixth dropped (frames {kept[0]}..{kept[-1]}), device-marked DwtDctSvd (scale 15, segments of {PER}), rotated by "
             f"{ANGLE} degree about the centre (float64 bilinear) and cropped to rows {ROWS[0]}:{ROWS[1]} / columns {COLS[0]}:{COLS[1]} ({h} x {w}); "
             f"routes alternating call by call, median of {args.reps} after {args.warmup} (min..max of the repetitions; spread = (max - min) / median), "
             f"kernel sources {source_sha16()}, {torch.cuda.get_device_name(0)}; ratio = row median / the median of the first row of its block",
             f"{'route':66s} {'median ms':>10s} {'min..max ms':>21s} {'spread':>7s} {'ratio':>7s}"]
    shown = [0]

    def show():
        for ln in lines[shown[0]:]:
            print(ln, flush=True)
        shown[0] = len(lines)

    show()
    # (a) the signatures of the whole library
    sig = torch.empty((N, 64), dtype=torch.uint8, device=dev)
    ref = [None]
    nbytes = library.numel() // 16 * 16
    sink = torch.zeros(4, dtype=torch.int32, device=dev)

    def fused_sig():
        eng.signatures(library, out=sig)

    def torch_sig():
        ref[0] = torch_signatures(library)

    def read_probe():
        _hip.check(eng.lib.ofmk_hbm_read(library.data_ptr(), nbytes, sink.data_ptr(), _hip.current_stream()))

    ms = alternate((fused_sig, read_probe, torch_sig), args.reps, args.warmup)
    assert torch.equal(sig, ref[0])
    gbs = [library.numel() / (float(np.median(ms[0])) * 1e6), nbytes / (float(np.median(ms[1])) * 1e6)]
    lines += [row(f"(a) signatures: one call, {N} frames", ms[0], float(np.median(ms[0]))),
              row("(a) ofmk_hbm_read of the same bytes (the read probe)", ms[1], float(np.median(ms[0]))),
              row("(a) same bytes: torch integer passes", ms[2], float(np.median(ms[0]))),
              "(a) " + verdict(ms[0], ms[2], "the call", "the torch passes") + f"; identical, all {N} x 64 bytes (asserted); {gbs[0]:.0f} GB/s of frame "
              f"bytes against {gbs[1]:.0f} GB/s of the read probe: {gbs[0] / gbs[1]:.2f} of the read rate; " + verdict(ms[0], ms[1], "the call", "the read probe")]
    show()
    del ref
    # (b) the distance matrix
    lsig = eng.signatures(leak)
    dist = torch.empty((m, N), dtype=torch.int32, device=dev)
    af, bf = lsig.float(), sig.float()
    cd = [None]

    def fused_dist():
        eng.signature_distances(lsig, sig, out=dist)

    def torch_dist():
        cd[0] = torch.cdist(af, bf, p=1)

    ms = alternate((fused_dist, torch_dist), args.reps, args.warmup)
    assert torch.equal(dist, cd[0].to(torch.int32)) and torch.equal(cd[0], cd[0].round())
    lines += [row(f"(b) signature_distances: one call, {m} x {N}", ms[0], float(np.median(ms[0]))),
              row("(b) torch.cdist(p=1) on float32 copies made beforehand", ms[1], float(np.median(ms[0]))),
              "(b) " + verdict(ms[0], ms[1], "the call", "torch.cdist") + f"; identical, all {m} x {N} integers (asserted)"]
    show()
    # (c) the residuals at the geometry registered on the true sources
    truth = np.asarray(kept, np.int64)
    k = 8
    geom = resync.register_leak(dec, library.index_select(0, torch.from_numpy(truth[:k]).to(dev)), leak[:k], (H, W))["geometry"]
    first = torch.from_numpy((truth - SPAN // 2).astype(np.int32)).to(dev)
    res = torch.empty((m, SPAN, 2), dtype=torch.int64, device=dev)
    comp = torch.empty((m, SPAN, 2), dtype=torch.int64, device=dev)
    g1 = torch.tensor([geom], dtype=torch.int64, device=dev)
    idx = [(first.to(torch.int64) + j) for j in range(SPAN)]

    def fused_res():
        eng.align_residuals(library, leak, first, SPAN, geom, out=res)

    def gathered_res():
        for j in range(SPAN):
            comp[:, j] = eng.align_sums(library.index_select(0, idx[j]), leak, g1)[:, 0, 27:29]

    ms = alternate((fused_res, gathered_res), args.reps, args.warmup)
    assert torch.equal(res, comp) and int(res[0, 0, 1]) > 0
    mse = (res[:, :, 0].double() / res[:, :, 1].double()).cpu().numpy()
    lines += [row(f"(c) align_residuals: one call, {m} frames, span {SPAN}", ms[0], float(np.median(ms[0]))),
              row(f"(c) same integers: {SPAN} x (index_select + align_sums)", ms[1], float(np.median(ms[0]))),
              "(c) " + verdict(ms[0], ms[1], "the call", "index_select + align_sums") + f"; identical, all {m} x {SPAN} x 2 integers (asserted); "
              f"sum e^2 / count at the true frame {mse[:, SPAN // 2].min():.2f}..{mse[:, SPAN // 2].max():.2f}, one frame off "
              f"{min(mse[:, SPAN // 2 - 1].min(), mse[:, SPAN // 2 + 1].min()):.2f}..{max(mse[:, SPAN // 2 - 1].max(), mse[:, SPAN // 2 + 1].max()):.2f}"]
    show()
    del comp, idx
    # (d) the whole recipe
    def whole():
        return temporal.read_leak_clip(dec, leak, library, PER, (H, W), cands, key=0, L=L, search_frames=k, span=SPAN, signatures=sig)

    def whole_with_signatures():
        return temporal.read_leak_clip(dec, leak, library, PER, (H, W), cands, key=0, L=L, search_frames=k, span=SPAN)

    ms_d, (got, got2) = alternate_wall((whole, whole_with_signatures), max(3, args.reps // 3), 1)
    coarse_err = np.abs(got["coarse_frame_map"] - truth)
    want = [chosen[s] for s in got["segments"]]
    lines += [row("(d) read_leak_clip, library signatures given, host time", ms_d[0], float(np.median(ms_d[0]))),
              row("(d) read_leak_clip, library signatures computed in the call", ms_d[1], float(np.median(ms_d[0]))),
              f"(d) coarse map: {int((coarse_err > 0).sum())} of {m} frames off, by at most {int(coarse_err.max())}; rounds {got['rounds_used']}; final "
              f"map exact for {int((got['frame_map'] == truth).sum())} of {m} frames; converged {got['registration']['converged']}, luma rms "
              f"{got['registration']['rms']:.3f}; residual at the map {got['residual'].min():.2f}..{got['residual'].max():.2f}; segments {got['segments']}, "
              f"copies {[int(p) for p in got['picks']]} (marked: {want}), ambiguous {got['ambiguous']}; the second form reads the same: "
              f"{bool(np.array_equal(got['frame_map'], got2['frame_map']) and got['geometry'] == got2['geometry'])}"]
    show()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
