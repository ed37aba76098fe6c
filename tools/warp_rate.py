"""Reading rescaled leaks (build extension), 8 x 1080p device-marked DwtDctSvd frames with a 16 px border cropped and resized back to
1080p (bench.py's attack crop16_and_resize_back): the two fused calls against the routes they replace --
  search  : ofmk_svd_warp_scores_rgb8 over K = 256 candidate geometries (one launch, no warped frame) vs
            PARENT route, what existed before the warp: per candidate torch.nn.functional.interpolate of the leak to the candidate's
                   crop size, the contiguous unit-aligned crop of that, svd_sync_scores(...)[:, 0]  (another resampler: its scores
                   are not the fused call's, only its cost is compared);
            CHAIN, the new calls one candidate at a time: warp of the counting rectangle + svd_sync_scores(...)[:, 0]  (asserted
                   identical to the fused call)
  readout : ofmk_svd_detect_soft_warp_rgb8 at the true geometry vs warp of the counting rectangle + svd_detect_soft_window
            (asserted identical)

The routes of a group alternate call by call in one process (stream events around one call); per row the median of --reps calls
after --warmup, the spread (min..max of the repetitions), and the row's median over the fused call's.  The verdict per baseline
says whether the fused call is faster beyond the spread: its slowest call beats the baseline's fastest.
Also printed: whether the leak now reads -- the geometry search's pick and read_rescaled_leak's copies at the known geometry.
usage: python tools/warp_rate.py [--frames 8] [--reps 30] [--warmup 2] [--out FILE]"""
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
from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder  # noqa: E402
from offmark.fingerprint import payload_for_segment  # noqa: E402
from offmark.generator.shuffler import Shuffler  # noqa: E402
from offmark.synthetic import synthetic_frames  # noqa: E402

L, BORDER, CHOSEN = 8, 16, (1, 0)


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

    def resized(x, h, w):                                   # bench.py's resize / back
        y = torch.nn.functional.interpolate(x.permute(0, 3, 1, 2).float(), size=(h, w), mode="bilinear", align_corners=False)
        return y.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    top, left, ch, cw = BORDER, BORDER, H - 2 * BORDER, W - 2 * BORDER
    leak = resized(marked[:, top:top + ch, left:left + cw], H, W)
    crops = [(t, l, hh, ww) for t in range(top - 2, top + 2) for l in range(left - 2, left + 2)
             for hh in range(ch - 2, ch + 2) for ww in range(cw - 2, cw + 2)]
    cands = resync.crop_candidates((H, W), (H, W), range(top - 2, top + 2), range(left - 2, left + 2), range(ch - 2, ch + 2),
                                   range(cw - 2, cw + 2))
    K = len(crops)
    assert cands.shape == (K, 4) and K == 256
    true_k = crops.index((top, left, ch, cw))
    cands_dev = torch.from_numpy(cands).to(dev)
    rects = [eng.warp_units((H, W), (H, W), g) for g in cands]
    res = [torch.zeros((n, K), dtype=torch.int64, device=dev) for _ in range(3)]

    def fused():
        eng.svd_warp_scores(leak, (H, W), cands_dev, scores=res[0])

    def parent():
        for k, (t, l, hh, ww) in enumerate(crops):
            back = resized(leak, hh, ww)                    # the candidate's crop, at canvas offset (t, l)
            y, x = -t % 8, -l % 8
            r, c = (hh - y) // 8, (ww - x) // 8
            res[1][:, k] = eng.svd_sync_scores(back[:, y:y + 8 * r, x:x + 8 * c].contiguous())[:, 0]

    def chain():
        for k, g in enumerate(cands):
            i0, i1, j0, j1 = rects[k]
            res[2][:, k] = eng.svd_sync_scores(eng.warp(leak, g, (8 * (i1 - i0), 8 * (j1 - j0)), origin=(8 * i0, 8 * j0)))[:, 0]

    g_true = cands[true_k]
    i0, i1, j0, j1 = rects[true_k]
    soft = [torch.empty((n, L), dtype=torch.int64, device=dev) for _ in range(2)]

    def fused_read():
        eng.svd_detect_soft_warp(leak, (H, W), g_true, L, soft=soft[0])

    def chain_read():
        rect = eng.warp(leak, g_true, (8 * (i1 - i0), 8 * (j1 - j0)), origin=(8 * i0, 8 * j0))
        eng.svd_detect_soft_window(rect, L, (0, 0), W // 8, base=i0 * (W // 8) + j0, soft=soft[1])

    lines = [f"# tools/warp_rate.py: {n} x {H}x{W} device-marked DwtDctSvd frames (scale 15), a {BORDER} px border cropped and resized back "
             f"(torch bilinear, half-pixel centres); search = K = {K} candidate geometries (crop edges -2..+1 px), readout = the true "
             f"geometry with L = {L}; routes of a group alternating call by call, median of {args.reps} after {args.warmup} (min..max of the "
             f"repetitions; spread = (max - min) / median), kernel sources {source_sha16()}, {torch.cuda.get_device_name(0)}; "
             f"ratio = row median / fused median",
             f"{'group':8s} {'route':34s} {'median ms':>10s} {'min..max ms':>21s} {'spread':>7s} {'ratio':>7s}"]
    print(lines[0])
    print(lines[1], flush=True)
    verdicts = []
    groups = (("search", (fused, parent, chain), ("fused warp scores", "parent: interpolate + crop + sync", "chain: warp + sync per candidate")),
              ("readout", (fused_read, chain_read), ("fused warp read-out", "chain: warp + soft window")))
    for group, routes, names in groups:
        ms = alternate(routes, args.reps, args.warmup)
        med = [float(np.median(m)) for m in ms]
        for name, m, t in zip(names, ms, med):
            lines.append(f"{group:8s} {name:34s} {t:10.3f} {m.min():10.3f}..{m.max():<10.3f} {100 * (m.max() - m.min()) / t:6.1f}% {t / med[0]:7.2f}")
            print(lines[-1], flush=True)
        for name, m, t in list(zip(names, ms, med))[1:]:
            if ms[0].max() < m.min():
                how = "IS faster beyond the spread than"
            elif m.max() < ms[0].min():
                how = "is SLOWER beyond the spread than"
            else:
                how = "is NOT beyond the spread of (medians " + ("faster" if med[0] < t else "slower") + ")"
            verdicts.append(f"{group}: the fused call {how} '{name}' (fused {ms[0].min():.3f}..{ms[0].max():.3f} ms, median {med[0]:.3f}; "
                            f"baseline {m.min():.3f}..{m.max():.3f} ms, median {t:.3f})")
    assert torch.equal(res[0], res[2]) and torch.equal(soft[0], soft[1])
    lines += verdicts
    lines.append("identical results: fused search == chain search, fused read-out == chain read-out (asserted); the parent route uses "
                 "another resampler and is compared by cost only")
    found = resync.best_geometry(res[0].cpu().numpy(), cands, (H, W), (H, W))
    found_parent = int(np.argmax(res[1].sum(dim=0).cpu().numpy() / np.array([((hh - (-t % 8)) // 8) * ((ww - (-l % 8)) // 8) for t, l, hh, ww in crops])))
    nrm = found["normalised"]
    lines.append(f"search: picks candidate {found['index']} (true: {true_k}), normalised {nrm[true_k]:.4f} at the true geometry against "
                 f"{np.delete(nrm, true_k).max():.4f} best other, contrast {found['contrast']:.3f}; the parent route's best mean score is "
                 f"candidate {found_parent}")
    cand_payloads = [[payload_for_segment(s + 1, c) for c in range(2)] for s in range(2)]
    got = resync.read_rescaled_leak(DwtDctSvdDecoder(), leak, seg, (H, W), cand_payloads, [g_true], key=0, L=L)
    plain = resync.align_segments(np.stack([eng.svd_detect_soft(leak, L).cpu().numpy()[seg == s].sum(axis=0) for s in range(2)]), cand_payloads, 0, bases=(0,))
    lines.append(f"crop{BORDER}_and_resize_back at its known geometry: copies {[int(p) for p in got['picks']]} (marked: {list(CHOSEN)}), score "
                 f"{got['score']}, ambiguous {got['ambiguous']}; the plain soft read-out of the same leak: copies {[int(p) for p in plain['picks']]}, "
                 f"score {plain['score']}")
    for ln in lines[-len(verdicts) - 3:]:
        print(ln)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
