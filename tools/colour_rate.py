"""Reading a leak whose colours changed (build extension): the two colour calls against the routes a user has without them, and
offmark.colour.read_coloured_leak against offmark.tone.read_toned_leak.  The workload is tools/tone_rate.py's -- 8 x 1080p
device-marked DwtDctSvd frames rotated by 1 degree about the centre on the host and cropped off-centre to 1001 x 1801; the sources are
the unmarked frames -- with the leak's pixels sent through clip(rint(M x), 0, 255), M = A709^-1 A601 (BT.601 pixels decoded as BT.709).
  (a) ofmk_colour_sums_rgb8 at K = 1 (the registered geometry) against ofmk_warp_affine_rgb8 of the canvas + torch integer passes
      (the mask, 1 + 6 + 15 + 6 masked products and sums per frame): asserted identical, all n x 28 integers; and against
      ofmk_tone_sums_rgb8 in the same loop (the same reads: the tile's taps and its source pixels)
  (b) ofmk_apply_colour_rgb8 against torch int32 passes (three multiply-adds, shift, clamp per channel, stacked; asserted identical),
      against ofmk_apply_tone_rgb8 and against the bytes it moves at the rate the copy probe (ofmk_hbm_copy) reaches in the same loop
  (c) the whole read_coloured_leak against read_toned_leak (host time, end to end), with the score and the copies each returns, and
      read_registered_leak on the same leak and on the leak before the colour map
The routes of a comparison alternate call by call in one process; per row the median of --reps calls after --warmup and the spread
(min..max of the repetitions).  A verdict is only given beyond the spread: one route's slowest call beats the other's fastest.
usage: python tools/colour_rate.py [--frames 8] [--reps 30] [--warmup 2] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-fingerprinting_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from affine_phase_rate import COLS, ROWS  # noqa: E402
from affine_rate import ANGLE, CHOSEN, L, rotate  # noqa: E402
from align_rate import alternate_wall, row, verdict  # noqa: E402
from copies_verify_rate import alternate, source_sha16  # noqa: E402
from offmark import _hip, colour, resync, tone  # noqa: E402
from offmark.engine import DctEngine  # noqa: E402
from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder  # noqa: E402
from offmark.fingerprint import payload_for_segment  # noqa: E402
from offmark.generator.shuffler import Shuffler  # noqa: E402
from offmark.synthetic import synthetic_frames  # noqa: E402

PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def ycbcr(w):
    """The full-range RGB -> YCbCr matrix of the luma weights w."""
    y = np.asarray(w, np.float64)
    return np.stack([y, (np.asarray([0.0, 0.0, 1.0]) - y) / (2.0 * (1.0 - w[2])), (np.asarray([1.0, 0.0, 0.0]) - y) / (2.0 * (1.0 - w[0]))])


M_601_AS_709 = np.linalg.inv(ycbcr((0.2126, 0.7152, 0.0722))) @ ycbcr((0.299, 0.587, 0.114))


def colour_map(frames, M):
    return np.ascontiguousarray(np.clip(np.rint(frames.astype(np.float64) @ M.T), 0, 255).astype(np.uint8))


def torch_colour_sums(eng, src, leak, geom, warped):
    """int64 [n, 28] from ofmk_warp_affine_rgb8 of the canvas and torch integer passes."""
    n, H, W = src.shape[:3]
    h, w = leak.shape[1:3]
    ayy, ayx, by, axy, axx, bx = (int(v) for v in geom)
    eng.warp_affine(leak, geom, (H, W), out=warped)
    y = torch.arange(H, dtype=torch.int64, device=src.device)[:, None]
    x = torch.arange(W, dtype=torch.int64, device=src.device)[None, :]
    y0, x0 = (ayy * y + ayx * x + by) >> 16, (axy * y + axx * x + bx) >> 16
    inside = (y0 >= 0) & (y0 <= h - 1) & (x0 >= 0) & (x0 <= w - 1)
    out = torch.zeros((n, 28), dtype=torch.int64, device=src.device)
    for f in range(n):
        ok = inside & ((warped[f] >= 1) & (warped[f] <= 254)).all(dim=2)
        lv, sv = warped[f][ok].to(torch.int64), src[f][ok].to(torch.int64)      # [pixels, 3]
        out[f, 0] = lv.shape[0]
        out[f, 1:4], out[f, 4:7] = lv.sum(dim=0), sv.sum(dim=0)
        for k, (i, j) in enumerate(PAIRS):
            out[f, 7 + k], out[f, 13 + k] = (lv[:, i] * lv[:, j]).sum(), (sv[:, i] * sv[:, j]).sum()
        for i in range(3):
            for j in range(3):
                out[f, 19 + 3 * i + j] = (lv[:, i] * sv[:, j]).sum()
    return out


def torch_apply_colour(frames, m):
    """uint8 [n, h, w, 3] from torch int32 passes; m: int32 [3, 4] on the device."""
    x = frames.to(torch.int32)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    return torch.stack([((m[c, 0] * r + m[c, 1] * g + m[c, 2] * b + (m[c, 3] + 32768)) >> 16).clamp_(0, 255) for c in range(3)], dim=-1).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, H, W = args.frames, 1080, 1920
    torch.cuda.set_device(0)
    eng = DctEngine()
    dev = eng.device
    dec = DwtDctSvdDecoder()
    seg = np.repeat(np.arange(2), (n + 1) // 2)[:n]
    wm = np.stack([Shuffler(key=0).generate_wm(payload_for_segment(s + 1, CHOSEN[s]), (H * W // 64,)) for s in range(2)]).astype(np.uint8)
    sources = synthetic_frames(n, H, W, seed=2000)
    marked = eng.svd_embed(sources, wm, wm_row=torch.from_numpy(seg.astype(np.int32)).to(dev))
    clean = np.ascontiguousarray(rotate(marked.cpu().numpy(), ANGLE)[:, ROWS[0]:ROWS[1], COLS[0]:COLS[1]])
    leak = torch.from_numpy(colour_map(clean, M_601_AS_709)).to(dev)
    clean = torch.from_numpy(clean).to(dev)
    h, w = int(leak.shape[1]), int(leak.shape[2])
    cand_payloads = [[payload_for_segment(s + 1, c) for c in range(2)] for s in range(2)]

    lines = [f"# tools/colour_rate.py: {n} x {H}x{W} device-marked DwtDctSvd frames (scale 15) rotated by {ANGLE} degree about the centre (host, "
             f"float64 bilinear, same size), cropped to rows {ROWS[0]}:{ROWS[1]} / columns {COLS[0]}:{COLS[1]} ({h} x {w}) and colour-mapped with "
             f"601as709 = {np.round(M_601_AS_709, 4).tolist()}; sources = the unmarked frames; routes alternating call by call, median of "
             f"{args.reps} after {args.warmup} (min..max of the repetitions; spread = (max - min) / median), kernel sources {source_sha16()}, "
             f"{torch.cuda.get_device_name(0)}; ratio = row median / the median of the first row of its block",
             f"{'route':66s} {'median ms':>10s} {'min..max ms':>21s} {'spread':>7s} {'ratio':>7s}"]
    shown = [0]

    def show():
        for ln in lines[shown[0]:]:
            print(ln, flush=True)
        shown[0] = len(lines)

    show()
    # the geometry the sums are taken at: the registration of the histogram-matched leak, as read_coloured_leak does it
    lut0 = tone.lut_of_histograms(eng.histograms(leak).sum(dim=0).cpu().numpy(), eng.histograms(sources).sum(dim=0).cpu().numpy())
    first = resync.register_leak(dec, sources, eng.apply_tone(leak, lut0), (H, W))
    geom = first["geometry"]
    lines += [f"# first registration (histogram-matched leak): converged {first['converged']}, iterations {first['iterations']}, luma rms "
              f"{first['rms']:.3f}, geometry {geom}"]

    # (a) the sums
    cands_dev = torch.tensor([geom], dtype=torch.int64, device=dev)
    fused = torch.zeros((n, 1, 28), dtype=torch.int64, device=dev)
    tsums = torch.zeros((n, 1, 3, 256, 2), dtype=torch.int64, device=dev)
    warped = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    composed = [None]

    def fused_call():
        eng.colour_sums(sources, leak, cands_dev, sums=fused)

    def composed_call():
        composed[0] = torch_colour_sums(eng, sources, leak, geom, warped)

    def tone_call():
        eng.tone_sums(sources, leak, cands_dev, sums=tsums)

    ms = alternate((fused_call, composed_call, tone_call), args.reps, args.warmup)
    assert torch.equal(fused[:, 0], composed[0]) and int(fused[0, 0, 0]) > 0
    inside = int(tsums[0, 0, 0, :, 0].sum())
    lines += [row(f"(a) colour_sums: one call, {n} frames, one geometry", ms[0], float(np.median(ms[0]))),
              row("(a) same sums: warp_affine of the canvas + torch integer passes", ms[1], float(np.median(ms[0]))),
              row("(a) tone_sums: one call, same frames and geometry", ms[2], float(np.median(ms[0]))),
              "(a) " + verdict(ms[0], ms[1], "the fused call", "warp_affine + torch") + f"; identical sums, all {n} x 28 integers (asserted); "
              f"{int(fused[0, 0, 0])} of the {inside} pixels inside the first frame contribute (the others hold a 0 or a 255)",
              "(a) " + verdict(ms[0], ms[2], "colour_sums", "tone_sums") + " (the same reads; 28 register sums against an LDS table)"]
    show()
    del composed, tsums

    # (b) the matrix
    matrix, fitted = colour.matrix_of_sums(fused.sum(dim=0)[0].cpu().numpy())
    m_dev = torch.from_numpy(matrix).to(dev)
    lut_dev = torch.from_numpy(lut0).to(dev)
    coloured, toned, passes = torch.empty_like(sources), torch.empty_like(sources), [None]
    nbytes = sources.numel()

    def apply_call():
        eng.apply_colour(sources, matrix, out=coloured)

    def torch_call():
        passes[0] = torch_apply_colour(sources, m_dev)

    def tone_apply_call():
        eng.apply_tone(sources, lut_dev, out=toned)

    def copy_probe():
        _hip.check(eng.lib.ofmk_hbm_copy(sources.data_ptr(), warped.data_ptr(), nbytes, _hip.current_stream()))

    ms = alternate((apply_call, torch_call, tone_apply_call, copy_probe), args.reps, args.warmup)
    assert torch.equal(coloured, passes[0])
    lines += [f"# the fitted matrix (Q16, fitted {fitted}): {matrix.tolist()}; residual rms {colour.residual_rms(fused.sum(dim=0)[0].cpu().numpy(), matrix):.3f}",
              row(f"(b) apply_colour: one call, {n} frames of {H}x{W}", ms[0], float(np.median(ms[0]))),
              row("(b) torch: int32 multiply-adds, shift, clamp per channel, stacked", ms[1], float(np.median(ms[0]))),
              row("(b) apply_tone of the same frames", ms[2], float(np.median(ms[0]))),
              row("(b) ofmk_hbm_copy of the same bytes (the copy probe)", ms[3], float(np.median(ms[0]))),
              "(b) " + verdict(ms[0], ms[1], "apply_colour", "the torch passes") + "; identical frames (asserted); " +
              verdict(ms[0], ms[3], "apply_colour", "the copy probe") + "; " + verdict(ms[0], ms[2], "apply_colour", "apply_tone") +
              f"; apply_colour reads and writes {nbytes / 1e6:.1f} MB each way: {2 * nbytes / np.median(ms[0]) / 1e6:.1f} GB/s at its median, the "
              f"copy probe {2 * nbytes / np.median(ms[3]) / 1e6:.1f} GB/s"]
    show()
    del coloured, toned, passes, warped
    torch.cuda.empty_cache()

    # (c) end to end
    def coloured_read():
        return colour.read_coloured_leak(dec, leak, sources, seg, (H, W), cand_payloads, key=0, L=L, search_frames=n)

    def toned_read():
        return tone.read_toned_leak(dec, leak, sources, seg, (H, W), cand_payloads, key=0, L=L, search_frames=n)

    reps_c = max(3, args.reps // 5)
    ms_c, (got, toned_got) = alternate_wall((coloured_read, toned_read), reps_c, 1)
    plain = resync.read_registered_leak(dec, leak, sources, seg, (H, W), cand_payloads, key=0, L=L, search_frames=n)
    untouched = resync.read_registered_leak(dec, clean, sources, seg, (H, W), cand_payloads, key=0, L=L, search_frames=n)

    def report(name, r):
        return (f"(c) {name}: copies {[int(p) for p in r['picks']]} (marked: {list(CHOSEN)}), score {r['score']}, ambiguous {r['ambiguous']}, converged "
                f"{r['registration']['converged']}, luma rms {r['registration']['rms']:.3f}, normalised {r['normalised']:.4f}, "
                f"{resync.corner_move(r['geometry'], untouched['geometry'], (H, W)):.3f} px from the untouched leak's geometry, "
                f"{r['score'] / untouched['score']:.3f} of its score")

    c = got["colour"]
    lines += [row(f"(c) read_coloured_leak, host time, end to end ({reps_c} repetitions)", ms_c[0], float(np.median(ms_c[0]))),
              row("(c) read_toned_leak on the same colour-mapped leak", ms_c[1], float(np.median(ms_c[0]))),
              "(c) " + verdict(ms_c[0], ms_c[1], "read_coloured_leak", "read_toned_leak") + " (both register twice)",
              report("read_coloured_leak", got) + f"; fitted {c['fitted']}, {c['pixels']} pixels, residual rms {c['residual_rms']:.3f}",
              report("read_toned_leak on the colour-mapped leak", toned_got), report("read_registered_leak on the colour-mapped leak", plain),
              report("read_registered_leak on the leak BEFORE the colour map", untouched)]
    show()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
