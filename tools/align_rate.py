"""Reading a leak against its SOURCE frames (build extension): registration in place of a geometry list.  The workload is
tools/affine_phase_rate.py's: 8 x 1080p device-marked DwtDctSvd frames rotated by 1 degree about the centre on the host and cropped
off-centre to 1001 x 1801; the sources are the unmarked frames.  Registration starts from offmark.resync.register_leak's default
start (centred, unrotated) with its default levels and is told nothing about the angle or the crop.
  (a) one full-resolution ofmk_align_sums_rgb8 call (8 frames, one geometry) against the same 29 sums from the calls that existed
      before it: ofmk_warp_affine_rgb8 of the canvas, then torch integer passes over it; asserted identical integer for integer
  (b) the whole register_leak (host time, synchronisations and the float64 solves included), with the iterations per level
  (c) read_registered_leak end to end against read_transformed_leak on tools/affine_phase_rate.py's K = 64 list -- a list that only
      spans +-0.15 degrees around the KNOWN angle, while registration assumes none
  (d) the normalised score and the copies at the registered geometry beside those at the list's best shifted geometry.
The routes of a comparison alternate call by call in one process; per row the median of --reps calls after --warmup and the spread
(min..max of the repetitions).  A verdict is only given beyond the spread: one route's slowest call beats the other's fastest.
usage: python tools/align_rate.py [--frames 8] [--reps 30] [--warmup 2] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-fingerprinting_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from affine_phase_rate import COLS, ROWS  # noqa: E402
from affine_rate import ANGLE, CHOSEN, L, rotate  # noqa: E402
from copies_verify_rate import alternate, source_sha16  # noqa: E402
from offmark import resync  # noqa: E402
from offmark.engine import DctEngine  # noqa: E402
from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder  # noqa: E402
from offmark.fingerprint import payload_for_segment  # noqa: E402
from offmark.generator.shuffler import Shuffler  # noqa: E402
from offmark.synthetic import synthetic_frames  # noqa: E402


def luma(t):
    p = t.to(torch.int64)
    return (p[..., 0] + 2 * p[..., 1] + p[..., 2] + 2) >> 2


def torch_sums(eng, src, leak, geom, warped):
    """The 29 sums of every frame from ofmk_warp_affine_rgb8 and torch integer passes: int64 [n, 29]."""
    n, H, W = src.shape[:3]
    h, w = leak.shape[1:3]
    ayy, ayx, by, axy, axx, bx = (int(v) for v in geom)
    eng.warp_affine(leak, geom, (H, W), out=warped)
    y = torch.arange(H, dtype=torch.int64, device=src.device)[:, None]
    x = torch.arange(W, dtype=torch.int64, device=src.device)[None, :]
    y0, x0 = (ayy * y + ayx * x + by) >> 16, (axy * y + axx * x + bx) >> 16
    ok = ((y0 >= 0) & (y0 <= h - 1) & (x0 >= 0) & (x0 <= w - 1))[1:-1, 1:-1].to(torch.int64)
    T, Yw = luma(src), luma(warped)
    gy = (T[:, 2:, 1:-1] - T[:, :-2, 1:-1]) * ok
    gx = (T[:, 1:-1, 2:] - T[:, 1:-1, :-2]) * ok
    e = (Yw - T)[:, 1:-1, 1:-1] * ok
    yc, xc = (y - (H >> 1))[1:-1], (x - (W >> 1))[:, 1:-1]
    sd = (gy * yc, gy * xc, gy, gx * yc, gx * xc, gx)
    out = [(sd[i] * sd[j]).sum(dim=(1, 2)) for i in range(6) for j in range(i, 6)]
    out += [(sd[i] * e).sum(dim=(1, 2)) for i in range(6)]
    out += [(e * e).sum(dim=(1, 2)), ok.sum().expand(n)]
    return torch.stack(out, dim=1)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def alternate_wall(routes, reps, warmup):
    """Host ms of every repetition of each route (synchronised before and after), the routes one after the other in every repetition;
    and each route's last result."""
    last = [None] * len(routes)
    for _ in range(warmup):
        for fn in routes:
            fn()
    ms = [[] for _ in routes]
    for _ in range(reps):
        for k, fn in enumerate(routes):
            t, last[k] = wall(fn)
            ms[k].append(t)
    return [np.asarray(m) for m in ms], last


def verdict(a, b, name_a, name_b):
    if a.max() < b.min():
        return f"{name_a} IS faster beyond the spread than {name_b}"
    if b.max() < a.min():
        return f"{name_a} is SLOWER beyond the spread than {name_b}"
    return f"{name_a} is NOT beyond the spread of {name_b} (medians " + ("faster" if np.median(a) < np.median(b) else "slower") + ")"


def row(name, m, base):
    t = float(np.median(m))
    return f"{name:66s} {t:10.3f} {m.min():10.3f}..{m.max():<10.3f} {100 * (m.max() - m.min()) / t:6.1f}% {t / base:7.2f}"


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
    leak = torch.from_numpy(np.ascontiguousarray(rotate(marked.cpu().numpy(), ANGLE)[:, ROWS[0]:ROWS[1], COLS[0]:COLS[1]])).to(dev)
    h, w = int(leak.shape[1]), int(leak.shape[2])
    start = resync.affine_of_rotation((H, W), (h, w), 0.0)
    levels = resync.default_levels((h, w))
    cand_payloads = [[payload_for_segment(s + 1, c) for c in range(2)] for s in range(2)]

    lines = [f"# tools/align_rate.py: {n} x {H}x{W} device-marked DwtDctSvd frames (scale 15) rotated by {ANGLE} degree about the centre (host, "
             f"float64 bilinear, same size) and cropped to rows {ROWS[0]}:{ROWS[1]} / columns {COLS[0]}:{COLS[1]} ({h} x {w}); sources = the "
             f"unmarked frames; registration from the centred unrotated start {start} with {levels} levels; routes alternating call by call, "
             f"median of {args.reps} after {args.warmup} (min..max of the repetitions; spread = (max - min) / median), kernel sources "
             f"{source_sha16()}, {torch.cuda.get_device_name(0)}; ratio = row median / the median of the first row of its block",
             f"{'route':66s} {'median ms':>10s} {'min..max ms':>21s} {'spread':>7s} {'ratio':>7s}"]

    shown = [0]

    def show():
        for ln in lines[shown[0]:]:
            print(ln, flush=True)
        shown[0] = len(lines)

    show()
    # (a) one full-resolution call against the calls that existed before it (stream events around one call)
    cands_dev = torch.tensor([start], dtype=torch.int64, device=dev)
    fused = torch.zeros((n, 1, 29), dtype=torch.int64, device=dev)
    warped = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    composed = [None]

    def fused_call():
        eng.align_sums(sources, leak, cands_dev, sums=fused)

    def composed_call():
        composed[0] = torch_sums(eng, sources, leak, start, warped)

    ms = alternate((fused_call, composed_call), args.reps, args.warmup)
    assert torch.equal(fused[:, 0], composed[0]) and int(fused[0, 0, 28]) > 0
    lines += [row("(a) align_sums: one call, 8 frames, one geometry", ms[0], float(np.median(ms[0]))),
              row("(a) same sums: warp_affine of the canvas + torch integer passes", ms[1], float(np.median(ms[0]))),
              "(a) " + verdict(ms[0], ms[1], "the fused call", "warp_affine + torch") + f"; identical sums, all {n} x 29 integers (asserted); "
              f"{int(fused[0, 0, 28])} contributing pixels per frame at the start"]
    show()
    del warped, composed
    torch.cuda.empty_cache()

    # (b) the whole registration
    ms_b, last = alternate_wall((lambda: resync.register_leak(dec, sources, leak, (H, W)),), max(3, args.reps // 3), 1)
    report = last[0]
    lines += [row("(b) register_leak, all frames, host time", ms_b[0], float(np.median(ms_b[0]))),
              f"(b) iterations per level, coarse to fine: {report['iterations']} ({sum(report['iterations'])} align_sums calls); converged "
              f"{report['converged']}; luma rms {report['rms']:.3f} over {report['pixels']} pixels; geometry {report['geometry']}, "
              f"{report['units']} counting units"]

    show()
    # (c) end to end against the list route of the parent commit
    angles = [ANGLE + 0.02 * d for d in range(-8, 8)]
    sub = resync.subpixel_shifts(2)
    listed = resync.rotation_candidates((H, W), (h, w), angles, [1.0], sub, sub)
    assert listed.shape[0] == 64

    def registered_read():
        return resync.read_registered_leak(dec, leak, sources, seg, (H, W), cand_payloads, key=0, L=L, search_frames=n)

    def listed_read():
        return resync.read_transformed_leak(dec, leak, seg, (H, W), cand_payloads, listed, key=0, L=L, search_frames=n)

    ms_c, (got, ref) = alternate_wall((registered_read, listed_read), args.reps, args.warmup)
    lines += [row("(c) read_registered_leak: no list, no angle given", ms_c[0], float(np.median(ms_c[0]))),
              row("(c) read_transformed_leak: K = 64 around the KNOWN angle", ms_c[1], float(np.median(ms_c[0]))),
              "(c) " + verdict(ms_c[0], ms_c[1], "read_registered_leak", "read_transformed_leak on its 64-entry list (+-0.15 degrees around the "
                               "known angle, half-pixel lattice)") + "; host time, end to end"]

    show()
    # (d) what each reads
    def normalised(geom):
        units = eng.affine_units((h, w), (H, W), geom)[4]
        s = eng.svd_affine_scores(leak, (H, W), np.asarray([geom], np.int64)).cpu().numpy().astype(np.int64)
        return float(s.sum()) / (resync.ONE * units * n), units

    truth = resync.shift_affine(listed[ref["index"]], *ref["phase"])
    (nr, ur), (nt, ut) = normalised(got["geometry"]), normalised(truth)
    lines += [f"(d) registered geometry: normalised {nr:.4f} on {ur} units, copies {[int(p) for p in got['picks']]} (marked: {list(CHOSEN)}), "
              f"score {got['score']}, ambiguous {got['ambiguous']}",
              f"(d) the list's best shifted geometry (entry {ref['index']}, phase {ref['phase']}): normalised {nt:.4f} on {ut} units, contrast "
              f"{ref['contrast']:.3f}, copies {[int(p) for p in ref['picks']]}, score {ref['score']}, ambiguous {ref['ambiguous']}; "
              f"{resync.corner_move(got['geometry'], truth, (H, W)):.3f} px between the two at the canvas corners"]
    show()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
