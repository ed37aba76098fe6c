"""Reading a leak whose brightness, contrast or gamma changed (build extension): the three tone calls against the routes a user has
without them, and offmark.tone.read_toned_leak against offmark.resync.read_registered_leak.  The workload is tools/align_rate.py's --
8 x 1080p device-marked DwtDctSvd frames rotated by 1 degree about the centre on the host and cropped off-centre to 1001 x 1801; the
sources are the unmarked frames -- with the leak's bytes sent through clip(rint(255 * (clip(a x + b, 0, 255) / 255) ** gamma), 0, 255),
(a, b, gamma) = (0.85, 15, 1).
  (a) ofmk_tone_sums_rgb8 at K = 1 (the registered geometry) against ofmk_warp_affine_rgb8 of the canvas + torch integer passes
      (bincount per frame and channel, plain and weighted by the source): asserted identical, all n x 3 x 256 x 2 integers
  (b) ofmk_histograms_rgb8 against torch.bincount per frame and channel: asserted identical
  (c) ofmk_apply_tone_rgb8 against torch.gather through the same table (asserted identical), against the bytes it moves at the rate
      the copy probe (ofmk_hbm_copy, reads and writes the same bytes) and the read probe (ofmk_hbm_read) reach in the same loop
  (d) the whole read_toned_leak against read_registered_leak (host time, end to end), with the score and the copies each returns
  (e) with --variants DIR: (a) and (b), and the same two calls on FLAT frames (every pixel of a tile in one bin: full contention), for
      every lib*.so in DIR -- the library built with other -DOFMK_TONE_RUNS / -DOFMK_TONE_WAVE_BINS / -DOFMK_TONE_HIST_COPIES
      (csrc/tone_kernels.hiph), the shipped library in the same loop; every result asserted identical to the shipped library's
The routes of a comparison alternate call by call in one process; per row the median of --reps calls after --warmup and the spread
(min..max of the repetitions).  A verdict is only given beyond the spread: one route's slowest call beats the other's fastest.
usage: python tools/tone_rate.py [--frames 8] [--reps 30] [--warmup 2] [--variants DIR] [--out FILE]"""
import argparse
import ctypes as C
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
from offmark import _hip, resync, tone  # noqa: E402
from offmark.engine import DctEngine  # noqa: E402
from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder  # noqa: E402
from offmark.fingerprint import payload_for_segment  # noqa: E402
from offmark.generator.shuffler import Shuffler  # noqa: E402
from offmark.synthetic import synthetic_frames  # noqa: E402

TONE = (0.85, 15.0, 1.0)


def tone_map(frames, a, b, gamma):
    x = np.clip(a * frames.astype(np.float64) + b, 0.0, 255.0)
    return np.ascontiguousarray(np.clip(np.rint(255.0 * (x / 255.0) ** gamma), 0, 255).astype(np.uint8))


def torch_hist(frames):
    """int64 [n, 3, 256] from torch.bincount per frame and channel."""
    return torch.stack([torch.stack([torch.bincount(f[:, :, c].reshape(-1).to(torch.int64), minlength=256) for c in range(3)]) for f in frames])


def torch_tone_sums(eng, src, leak, geom, warped):
    """int64 [n, 3, 256, 2] from ofmk_warp_affine_rgb8 of the canvas and torch integer passes."""
    n, H, W = src.shape[:3]
    h, w = leak.shape[1:3]
    ayy, ayx, by, axy, axx, bx = (int(v) for v in geom)
    eng.warp_affine(leak, geom, (H, W), out=warped)
    y = torch.arange(H, dtype=torch.int64, device=src.device)[:, None]
    x = torch.arange(W, dtype=torch.int64, device=src.device)[None, :]
    y0, x0 = (ayy * y + ayx * x + by) >> 16, (axy * y + axx * x + bx) >> 16
    inside = ((y0 >= 0) & (y0 <= h - 1) & (x0 >= 0) & (x0 <= w - 1)).reshape(-1)
    out = torch.zeros((n, 3, 256, 2), dtype=torch.int64, device=src.device)
    for f in range(n):
        for c in range(3):
            v = warped[f, :, :, c].reshape(-1)[inside].to(torch.int64)
            s = src[f, :, :, c].reshape(-1)[inside].to(torch.int64)
            out[f, c, :, 0] = torch.bincount(v, minlength=256)
            out[f, c, :, 1].index_add_(0, v, s)
    return out


class Variant:
    """Another build of the library, loaded beside the shipped one: the two reduction calls through raw pointers."""

    def __init__(self, path):
        self.name = os.path.basename(path)[3:-3].lstrip("_")
        self.lib = C.CDLL(path)
        for name in ("ofmk_histograms_rgb8", "ofmk_tone_sums_rgb8"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _hip.SIGNATURES[name]

    def histograms(self, frames, out):
        n, h, w = frames.shape[:3]
        assert self.lib.ofmk_histograms_rgb8(frames.data_ptr(), n, h, w, out.data_ptr(), _hip.current_stream(), None) == 0

    def tone_sums(self, src, leak, cands, out):
        n, H, W = src.shape[:3]
        h, w = leak.shape[1:3]
        assert self.lib.ofmk_tone_sums_rgb8(src.data_ptr(), leak.data_ptr(), n, h, w, H, W, cands.data_ptr(), int(cands.shape[0]), out.data_ptr(),
                                            _hip.current_stream(), None) == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--variants", default=None)
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
    leak = torch.from_numpy(tone_map(clean, *TONE)).to(dev)
    clean = torch.from_numpy(clean).to(dev)
    h, w = int(leak.shape[1]), int(leak.shape[2])
    cand_payloads = [[payload_for_segment(s + 1, c) for c in range(2)] for s in range(2)]

    lines = [f"# tools/tone_rate.py: {n} x {H}x{W} device-marked DwtDctSvd frames (scale 15) rotated by {ANGLE} degree about the centre (host, "
             f"float64 bilinear, same size), cropped to rows {ROWS[0]}:{ROWS[1]} / columns {COLS[0]}:{COLS[1]} ({h} x {w}) and tone-mapped with "
             f"(a, b, gamma) = {TONE}; sources = the unmarked frames; routes alternating call by call, median of {args.reps} after {args.warmup} "
             f"(min..max of the repetitions; spread = (max - min) / median), kernel sources {source_sha16()}, {torch.cuda.get_device_name(0)}; "
             f"ratio = row median / the median of the first row of its block",
             f"{'route':66s} {'median ms':>10s} {'min..max ms':>21s} {'spread':>7s} {'ratio':>7s}"]
    shown = [0]

    def show():
        for ln in lines[shown[0]:]:
            print(ln, flush=True)
        shown[0] = len(lines)

    show()
    # the geometry the sums are taken at: the registration of the histogram-matched leak, as read_toned_leak does it
    lut0 = tone.lut_of_histograms(eng.histograms(leak).sum(dim=0).cpu().numpy(), eng.histograms(sources).sum(dim=0).cpu().numpy())
    first = resync.register_leak(dec, sources, eng.apply_tone(leak, lut0), (H, W))
    geom = first["geometry"]
    lines += [f"# first registration (histogram-matched leak): converged {first['converged']}, iterations {first['iterations']}, luma rms "
              f"{first['rms']:.3f}, geometry {geom}"]

    # (a) the conditional sums
    cands_dev = torch.tensor([geom], dtype=torch.int64, device=dev)
    fused = torch.zeros((n, 1, 3, 256, 2), dtype=torch.int64, device=dev)
    warped = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    composed = [None]

    def fused_call():
        eng.tone_sums(sources, leak, cands_dev, sums=fused)

    def composed_call():
        composed[0] = torch_tone_sums(eng, sources, leak, geom, warped)

    ms = alternate((fused_call, composed_call), args.reps, args.warmup)
    assert torch.equal(fused[:, 0], composed[0]) and int(fused[0, 0, 0, :, 0].sum()) > 0
    lines += [row(f"(a) tone_sums: one call, {n} frames, one geometry", ms[0], float(np.median(ms[0]))),
              row("(a) same sums: warp_affine of the canvas + torch bincount / index_add_", ms[1], float(np.median(ms[0]))),
              "(a) " + verdict(ms[0], ms[1], "the fused call", "warp_affine + torch") + f"; identical sums, all {n} x 3 x 256 x 2 integers "
              f"(asserted); {int(fused[0, 0, 0, :, 0].sum())} pixels inside per frame, {int((fused[0, 0, :, :, 0] > 0).sum())} of 768 bins populated"]
    show()
    del composed

    # (b) the histograms
    hist = torch.zeros((n, 3, 256), dtype=torch.int64, device=dev)
    ref = [None]

    def hist_call():
        eng.histograms(sources, out=hist)

    def bincount_call():
        ref[0] = torch_hist(sources)

    ms = alternate((hist_call, bincount_call), args.reps, args.warmup)
    assert torch.equal(hist, ref[0])
    nbytes = sources.numel()
    lines += [row(f"(b) histograms: one call, {n} frames of {H}x{W}", ms[0], float(np.median(ms[0]))),
              row("(b) torch.bincount per frame and channel", ms[1], float(np.median(ms[0]))),
              "(b) " + verdict(ms[0], ms[1], "the call", "torch.bincount") + f"; identical histograms (asserted); {nbytes / np.median(ms[0]) / 1e6:.1f} "
              "GB/s of frame bytes at the call's median"]
    show()

    # (c) the table
    lut = tone.lut_of_sums(fused.sum(dim=0)[0].cpu().numpy())
    lut_dev = torch.from_numpy(lut).to(dev)
    toned, gathered = torch.empty_like(sources), [None]
    sink = torch.zeros(64, dtype=torch.int32, device=dev)

    def apply_call():
        eng.apply_tone(sources, lut_dev, out=toned)

    def gather_call():
        gathered[0] = torch.stack([lut_dev[c][sources[..., c].to(torch.int64)] for c in range(3)], dim=-1)

    def copy_probe():
        _hip.check(eng.lib.ofmk_hbm_copy(sources.data_ptr(), warped.data_ptr(), nbytes, _hip.current_stream()))

    def read_probe():
        _hip.check(eng.lib.ofmk_hbm_read(sources.data_ptr(), nbytes, sink.data_ptr(), _hip.current_stream()))

    ms = alternate((apply_call, gather_call, copy_probe, read_probe), args.reps, args.warmup)
    assert torch.equal(toned, gathered[0])
    lines += [row(f"(c) apply_tone: one call, {n} frames of {H}x{W}", ms[0], float(np.median(ms[0]))),
              row("(c) torch: a gather through the table per channel, stacked", ms[1], float(np.median(ms[0]))),
              row("(c) ofmk_hbm_copy of the same bytes (the copy probe)", ms[2], float(np.median(ms[0]))),
              row("(c) ofmk_hbm_read of the same bytes (the read probe)", ms[3], float(np.median(ms[0]))),
              "(c) " + verdict(ms[0], ms[1], "apply_tone", "the torch gather") + "; identical frames (asserted); " +
              verdict(ms[0], ms[2], "apply_tone", "the copy probe") + f"; apply_tone reads and writes {nbytes / 1e6:.1f} MB each way: "
              f"{2 * nbytes / np.median(ms[0]) / 1e6:.1f} GB/s at its median, the copy probe {2 * nbytes / np.median(ms[2]) / 1e6:.1f} GB/s, the read "
              f"probe {nbytes / np.median(ms[3]) / 1e6:.1f} GB/s"]
    show()
    del toned, gathered, warped
    torch.cuda.empty_cache()

    # (d) end to end
    def toned_read():
        return tone.read_toned_leak(dec, leak, sources, seg, (H, W), cand_payloads, key=0, L=L, search_frames=n)

    def plain_read():
        return resync.read_registered_leak(dec, leak, sources, seg, (H, W), cand_payloads, key=0, L=L, search_frames=n)

    reps_d = max(3, args.reps // 5)
    ms_d, (got, plain) = alternate_wall((toned_read, plain_read), reps_d, 1)
    untouched = resync.read_registered_leak(dec, clean, sources, seg, (H, W), cand_payloads, key=0, L=L, search_frames=n)
    lines += [row(f"(d) read_toned_leak, host time, end to end ({reps_d} repetitions)", ms_d[0], float(np.median(ms_d[0]))),
              row("(d) read_registered_leak on the same tone-mapped leak", ms_d[1], float(np.median(ms_d[0]))),
              "(d) " + verdict(ms_d[0], ms_d[1], "read_toned_leak", "read_registered_leak") + " (it registers twice and adds the tone calls)",
              f"(d) read_toned_leak: copies {[int(p) for p in got['picks']]} (marked: {list(CHOSEN)}), score {got['score']}, ambiguous {got['ambiguous']}, "
              f"converged {got['registration']['converged']}, luma rms {got['registration']['rms']:.3f}, normalised {got['normalised']:.4f}",
              f"(d) read_registered_leak on the tone-mapped leak: copies {[int(p) for p in plain['picks']]}, score {plain['score']}, ambiguous "
              f"{plain['ambiguous']}, converged {plain['registration']['converged']}, luma rms {plain['registration']['rms']:.3f}, normalised "
              f"{plain['normalised']:.4f}; {resync.corner_move(plain['geometry'], got['geometry'], (H, W)):.3f} px from read_toned_leak's geometry",
              f"(d) read_registered_leak on the leak BEFORE the tone map: copies {[int(p) for p in untouched['picks']]}, score {untouched['score']}, "
              f"luma rms {untouched['registration']['rms']:.3f}, normalised {untouched['normalised']:.4f}; "
              f"{resync.corner_move(untouched['geometry'], got['geometry'], (H, W)):.3f} px from read_toned_leak's geometry; the tone fit's score is "
              f"{got['score'] / untouched['score']:.3f} of it"]
    show()

    # (e) other builds of the two reduction kernels
    if args.variants:
        paths = sorted(os.path.join(args.variants, f) for f in os.listdir(args.variants) if f.startswith("lib") and f.endswith(".so"))
        variants = [Variant(p) for p in paths]
        flat_leak, flat_src = torch.full_like(leak, 200), torch.full_like(sources, 100)
        flat_leak[1::2, :, :, 1] = 3
        outs = [torch.zeros_like(fused) for _ in variants]
        houts = [torch.zeros_like(hist) for _ in variants]
        for what, s, f in (("the workload", sources, leak), ("FLAT frames", flat_src, flat_leak)):
            routes = [lambda: eng.tone_sums(s, f, cands_dev, sums=fused)] + [lambda v=v, o=o: v.tone_sums(s, f, cands_dev, o) for v, o in zip(variants, outs)]
            ms = alternate(routes, args.reps, args.warmup)
            assert all(torch.equal(o, fused) for o in outs)
            lines += [row(f"(e) tone_sums on {what}: the shipped library", ms[0], float(np.median(ms[0])))]
            lines += [row(f"(e) tone_sums on {what}: {v.name}", m, float(np.median(ms[0]))) for v, m in zip(variants, ms[1:])]
            routes = [lambda: eng.histograms(s, out=hist)] + [lambda v=v, o=o: v.histograms(s, o) for v, o in zip(variants, houts)]
            ms = alternate(routes, args.reps, args.warmup)
            assert all(torch.equal(o, hist) for o in houts)
            lines += [row(f"(e) histograms on {what}: the shipped library", ms[0], float(np.median(ms[0])))]
            lines += [row(f"(e) histograms on {what}: {v.name}", m, float(np.median(ms[0]))) for v, m in zip(variants, ms[1:])]
            show()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
