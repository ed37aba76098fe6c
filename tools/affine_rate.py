"""Reading rotated leaks (build extension), 8 x 1080p device-marked DwtDctSvd frames rotated by 1 degree about the centre on the host
(float64 bilinear, same size): the fused calls against the routes they replace --
  search  : ofmk_svd_affine_scores_rgb8 over K = 256 candidate geometries (16 angles in 0.02 degree steps around the truth x 4 x 4
            whole-pixel shifts; one launch, no warped frame) vs
            PARENT route, what a user could do before the affine calls: per candidate torch.nn.functional.affine_grid + grid_sample
                   of the leak onto the canvas, svd_detect_soft with one position per unit, the counting units as a mask,
                   abs().sum()  (another resampler: its scores are not the fused call's, only its cost is compared);
            CHAIN, the new calls one candidate at a time: warp_affine of the canvas + svd_detect_soft + mask + abs().sum()
                   (asserted identical to the fused call);
  general : the same list with its off-diagonal terms zeroed through ofmk_svd_affine_scores_rgb8 vs the 4-parameter
            ofmk_svd_warp_scores_rgb8 (asserted identical): the price of generality
  readout : ofmk_svd_detect_soft_affine_rgb8 at the true geometry vs warp_affine of the bounding rectangle + svd_detect_soft
            + mask + regroup at the canvas positions (asserted identical)

The routes of a group alternate call by call in one process (stream events around one call); per row the median of --reps calls
after --warmup, the spread (min..max of the repetitions), and the row's median over the fused call's.  The verdict per baseline
says whether the fused call is faster beyond the spread: its slowest call beats the baseline's fastest.
Also printed: whether the truth ranks first, and its contrast.
usage: python tools/affine_rate.py [--frames 8] [--reps 30] [--warmup 2] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-fingerprinting_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from copies_verify_rate import alternate, source_sha16  # noqa: E402
from offmark import resync  # noqa: E402
from offmark.engine import DctEngine  # noqa: E402
from offmark.fingerprint import payload_for_segment  # noqa: E402
from offmark.generator.shuffler import Shuffler  # noqa: E402
from offmark.synthetic import synthetic_frames  # noqa: E402

L, ANGLE, CHOSEN = 8, 1.0, (1, 0)


def rotate(frames, angle_deg):
    """u8 [n, H, W, 3] on the host: pixel p samples the frame at R(angle) (p - c) + c, clamped into the frame; float64 bilinear,
    rint, clip -- what offmark.resync.affine_of_rotation inverts."""
    H, W = frames.shape[1:3]
    a = np.deg2rad(angle_deg)
    dy, dx = np.arange(H, dtype=np.float64)[:, None] - (H - 1) / 2.0, np.arange(W, dtype=np.float64)[None, :] - (W - 1) / 2.0
    sy = np.clip(np.cos(a) * dy - np.sin(a) * dx + (H - 1) / 2.0, 0.0, H - 1.0)
    sx = np.clip(np.sin(a) * dy + np.cos(a) * dx + (W - 1) / 2.0, 0.0, W - 1.0)
    y0, x0 = np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    fy, fx = (sy - y0)[:, :, None], (sx - x0)[:, :, None]
    out = np.empty_like(frames)
    for k, f in enumerate(frames):
        p = f.astype(np.float64)
        top = (1 - fx) * p[y0, x0] + fx * p[y0, x1]
        bot = (1 - fx) * p[y1, x0] + fx * p[y1, x1]
        out[k] = np.clip(np.rint((1 - fy) * top + fy * bot), 0, 255).astype(np.uint8)
    return out


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
    seg = np.repeat(np.arange(2), (n + 1) // 2)[:n]
    wm = np.stack([Shuffler(key=0).generate_wm(payload_for_segment(s + 1, CHOSEN[s]), (H * W // 64,)) for s in range(2)]).astype(np.uint8)
    marked = eng.svd_embed(synthetic_frames(n, H, W, seed=2000), wm, wm_row=torch.from_numpy(seg.astype(np.int32)).to(dev))
    leak = torch.from_numpy(rotate(marked.cpu().numpy(), ANGLE)).to(dev)

    angles = [ANGLE + 0.02 * d for d in range(-8, 8)]
    shifts = [-1.0, 0.0, 1.0, 2.0]
    cands = resync.rotation_candidates((H, W), (H, W), angles, [1.0], shifts, shifts)
    K = cands.shape[0]
    assert K == 256
    true_k = [tuple(c) for c in cands].index(resync.affine_of_rotation((H, W), (H, W), ANGLE))
    cands_dev = torch.from_numpy(cands).to(dev)
    units = (H // 8) * (W // 8)
    masks = torch.from_numpy(np.stack([resync.affine_units((H, W), (H, W), g).reshape(-1) for g in cands])).to(dev)
    res = [torch.zeros((n, K), dtype=torch.int64, device=dev) for _ in range(3)]
    per_unit = torch.empty((n, units), dtype=torch.int64, device=dev)
    canvas = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)

    # the parent route's sampling grids: theta of affine_grid (align_corners=True) from the same Q16 maps
    q = cands.astype(np.float64) / 65536.0
    sy, sx = 2.0 / (H - 1), 2.0 / (W - 1)
    theta = np.empty((K, 2, 3))
    theta[:, 0, 0], theta[:, 0, 1] = q[:, 4], q[:, 3] * sx / sy
    theta[:, 0, 2] = sx * (q[:, 5] + q[:, 3] / sy + q[:, 4] / sx) - 1
    theta[:, 1, 0], theta[:, 1, 1] = q[:, 1] * sy / sx, q[:, 0]
    theta[:, 1, 2] = sy * (q[:, 2] + q[:, 0] / sy + q[:, 1] / sx) - 1
    theta_dev = torch.from_numpy(theta).float().to(dev)

    def fused():
        eng.svd_affine_scores(leak, (H, W), cands_dev, scores=res[0])

    def parent():
        src = leak.permute(0, 3, 1, 2).float()
        for k in range(K):
            grid = torch.nn.functional.affine_grid(theta_dev[k:k + 1].expand(n, 2, 3), (n, 3, H, W), align_corners=True)
            y = torch.nn.functional.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
            back = y.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
            res[1][:, k] = (eng.svd_detect_soft(back, units, soft=per_unit).abs() * masks[k]).sum(dim=1)

    def chain():
        for k in range(K):
            eng.warp_affine(leak, cands[k], (H, W), out=canvas)
            res[2][:, k] = (eng.svd_detect_soft(canvas, units, soft=per_unit).abs() * masks[k]).sum(dim=1)

    routes, names = [fused, parent, chain], ["fused affine scores", "parent: affine_grid + grid_sample + soft",
                                             "chain: warp_affine + soft per candidate"]
    zero = cands.copy()
    zero[:, 1] = zero[:, 3] = 0
    zero_dev = torch.from_numpy(zero).to(dev)
    four_dev = torch.from_numpy(np.ascontiguousarray(zero[:, [0, 2, 4, 5]])).to(dev)
    gen = [torch.zeros((n, K), dtype=torch.int64, device=dev) for _ in range(2)]

    def general():
        eng.svd_affine_scores(leak, (H, W), zero_dev, scores=gen[0])

    def four():
        eng.svd_warp_scores(leak, (H, W), four_dev, scores=gen[1])

    g_true = cands[true_k]
    i0, i1, j0, j1, count = eng.affine_units((H, W), (H, W), g_true)
    rows, cols = i1 - i0, j1 - j0
    rect_mask = masks[true_k].reshape(H // 8, W // 8)[i0:i1, j0:j1].reshape(-1)
    ii, jj = np.divmod(np.arange(rows * cols), cols)
    positions = torch.from_numpy(((i0 + ii) * (W // 8) + j0 + jj) % L).to(dev)
    soft = [torch.empty((n, L), dtype=torch.int64, device=dev) for _ in range(2)]
    rect = torch.empty((n, 8 * rows, 8 * cols, 3), dtype=torch.uint8, device=dev)
    rect_units = torch.empty((n, rows * cols), dtype=torch.int64, device=dev)

    def fused_read():
        eng.svd_detect_soft_affine(leak, (H, W), g_true, L, soft=soft[0])

    def chain_read():
        eng.warp_affine(leak, g_true, (8 * rows, 8 * cols), origin=(8 * i0, 8 * j0), out=rect)
        m = eng.svd_detect_soft(rect, rows * cols, soft=rect_units) * rect_mask
        soft[1].zero_().index_add_(1, positions, m)

    lines = [f"# tools/affine_rate.py: {n} x {H}x{W} device-marked DwtDctSvd frames (scale 15) rotated by {ANGLE} degree about the centre "
             f"(host, float64 bilinear, same size); search = K = {K} candidate geometries ({len(angles)} angles in 0.02 degree steps x "
             f"{len(shifts)} x {len(shifts)} shifts of -1..2 px), general = the same list with zero off-diagonal terms, readout = the true "
             f"geometry ({count} counting units in a {rows} x {cols} rectangle) with L = {L}; routes of a group alternating call by call, "
             f"median of {args.reps} after {args.warmup} (min..max of the repetitions; spread = (max - min) / median), kernel sources "
             f"{source_sha16()}, {torch.cuda.get_device_name(0)}; ratio = row median / fused median",
             f"{'group':8s} {'route':42s} {'median ms':>10s} {'min..max ms':>21s} {'spread':>7s} {'ratio':>7s}"]
    print(lines[0])
    print(lines[1], flush=True)
    verdicts = []
    groups = (("search", routes, names),
              ("general", (general, four), ("fused affine scores, zero off-diagonals", "4-parameter fused warp scores")),
              ("readout", (fused_read, chain_read), ("fused affine read-out", "chain: warp_affine + soft + regroup")))
    for group, fns, labels in groups:
        ms = alternate(fns, args.reps, args.warmup)
        med = [float(np.median(m)) for m in ms]
        for name, m, t in zip(labels, ms, med):
            lines.append(f"{group:8s} {name:42s} {t:10.3f} {m.min():10.3f}..{m.max():<10.3f} {100 * (m.max() - m.min()) / t:6.1f}% {t / med[0]:7.2f}")
            print(lines[-1], flush=True)
        for name, m, t in list(zip(labels, ms, med))[1:]:
            if ms[0].max() < m.min():
                how = "IS faster beyond the spread than"
            elif m.max() < ms[0].min():
                how = "is SLOWER beyond the spread than"
            else:
                how = "is NOT beyond the spread of (medians " + ("faster" if med[0] < t else "slower") + ")"
            verdicts.append(f"{group}: the fused call {how} '{name}' (fused {ms[0].min():.3f}..{ms[0].max():.3f} ms, median {med[0]:.3f}; "
                            f"baseline {m.min():.3f}..{m.max():.3f} ms, median {t:.3f})")
    assert torch.equal(res[0], res[2]) and torch.equal(gen[0], gen[1]) and torch.equal(soft[0], soft[1])
    lines += verdicts
    lines.append("identical results: fused search == chain search, affine == 4-parameter "
                 "scores at zero off-diagonals, fused read-out == chain read-out (asserted); the parent route uses another resampler and is "
                 "compared by cost only")
    found = resync.best_geometry(res[0].cpu().numpy(), cands, (H, W), (H, W))
    nrm = found["normalised"]
    unit_counts = masks.sum(dim=1).cpu().numpy()
    found_parent = int(np.argmax(res[1].sum(dim=0).cpu().numpy() / unit_counts))
    lines.append(f"search: picks candidate {found['index']} (true: {true_k}), normalised {nrm[true_k]:.4f} at the true geometry against "
                 f"{np.delete(nrm, true_k).max():.4f} best other, contrast {found['contrast']:.3f}; the parent route's best mean score is "
                 f"candidate {found_parent}")
    cand_payloads = [[payload_for_segment(s + 1, c) for c in range(2)] for s in range(2)]
    by_segment = np.stack([soft[0].cpu().numpy()[seg == s].sum(axis=0) for s in range(2)])
    got = resync.align_segments(by_segment, cand_payloads, 0, bases=(0,))
    lines.append(f"read-out at the true geometry: copies {[int(p) for p in got['picks']]} (marked: {list(CHOSEN)}), score {got['score']}, "
                 f"ambiguous {got['ambiguous']}")
    for ln in lines[-len(verdicts) - 3:]:
        print(ln)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
