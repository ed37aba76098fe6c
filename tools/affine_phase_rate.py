"""Reading rotated-AND-cropped leaks (build extension), 8 x 1080p device-marked DwtDctSvd frames rotated by 1 degree about the
centre on the host (tools/affine_rate.py: float64 bilinear, same size) and then cropped off-centre to odd sizes, so that the
translation is unknown:
  dense   : ofmk_svd_affine_phase_scores_rgb8 over K = 64 list entries (16 angles in 0.02 degree steps around the truth x
            offmark.resync.subpixel_shifts(2) squared), all 64 whole-pixel shifts of each inside the call: 4096 shifted geometries
  listed  : the parent commit's route to the same 4096 numbers: ofmk_svd_affine_scores_rgb8 over the 4096 shifted candidates
            (offmark.resync.shift_affine of every entry and shift), asserted identical integer for integer.
The two routes alternate call by call in one process (stream events around one call); per row the median of --reps calls after
--warmup, the spread (min..max of the repetitions) and the row's median over the dense call's.  The verdict says whether the
dense call is faster beyond the spread: its slowest call beats the baseline's fastest.
Also printed: the truth's rank and both contrasts of best_shifted_geometry on that leak, and the copies read_transformed_leak
returns.
usage: python tools/affine_phase_rate.py [--frames 8] [--reps 30] [--warmup 2] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-fingerprinting_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from affine_rate import ANGLE, CHOSEN, L, rotate  # noqa: E402
from copies_verify_rate import alternate, source_sha16  # noqa: E402
from offmark import resync  # noqa: E402
from offmark.engine import DctEngine  # noqa: E402
from offmark.extract.dwt_dct_svd_decoder import DwtDctSvdDecoder  # noqa: E402
from offmark.fingerprint import payload_for_segment  # noqa: E402
from offmark.generator.shuffler import Shuffler  # noqa: E402
from offmark.synthetic import synthetic_frames  # noqa: E402

ROWS, COLS = (37, 1038), (53, 1854)          # the crop of the rotated frames: 1001 x 1801, centre 2.5 / 6.5 px off the frame's


def expected(H, W, sub):
    """The list's sub-pixel shift and the whole-pixel phase nearest to the leak's true translation R(angle) * (crop centre - frame
    centre): -> (sub_y, sub_x), (py, px), the residual in px."""
    a = np.deg2rad(ANGLE)
    d = np.array([(ROWS[0] + ROWS[1] - 1) / 2.0 - (H - 1) / 2.0, (COLS[0] + COLS[1] - 1) / 2.0 - (W - 1) / 2.0])
    t = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]) @ d
    best = None
    for sy in sub:
        for sx in sub:
            m = np.rint(t - (sy, sx))
            err = float(np.abs(t - (sy, sx) - m).max())
            if best is None or err < best[2]:
                best = ((sy, sx), (int(-m[0]) % 8, int(-m[1]) % 8), err)
    return best


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
    leak = torch.from_numpy(np.ascontiguousarray(rotate(marked.cpu().numpy(), ANGLE)[:, ROWS[0]:ROWS[1], COLS[0]:COLS[1]])).to(dev)
    h, w = int(leak.shape[1]), int(leak.shape[2])

    angles = [ANGLE + 0.02 * d for d in range(-8, 8)]
    sub = resync.subpixel_shifts(2)
    cands = resync.rotation_candidates((H, W), (h, w), angles, [1.0], sub, sub)
    K = cands.shape[0]
    assert K == 64
    true_sub, true_phase, residual = expected(H, W, sub)
    true_k = [tuple(c) for c in cands].index(resync.affine_of_rotation((H, W), (h, w), ANGLE, 1.0, true_sub))
    cands_dev = torch.from_numpy(cands).to(dev)
    shifted = np.stack([resync.shift_affine(cands, py, px) for py in range(8) for px in range(8)], axis=1).reshape(K * 64, 6)
    shifted_dev = torch.from_numpy(np.ascontiguousarray(shifted)).to(dev)
    dense = torch.zeros((n, K, 64), dtype=torch.int64, device=dev)
    units = torch.zeros((K, 64), dtype=torch.int64, device=dev)
    listed = torch.zeros((n, K * 64), dtype=torch.int64, device=dev)

    def dense_call():
        eng.svd_affine_phase_scores(leak, (H, W), cands_dev, scores=dense, units=units)

    def listed_call():
        eng.svd_affine_scores(leak, (H, W), shifted_dev, scores=listed)

    lines = [f"# tools/affine_phase_rate.py: {n} x {H}x{W} device-marked DwtDctSvd frames (scale 15) rotated by {ANGLE} degree about the centre "
             f"(host, float64 bilinear, same size) and cropped to rows {ROWS[0]}:{ROWS[1]} / columns {COLS[0]}:{COLS[1]} ({h} x {w}); list = K = {K} "
             f"entries ({len(angles)} angles in 0.02 degree steps x subpixel_shifts(2) squared), {K * 64} shifted geometries; the two routes "
             f"alternating call by call, median of {args.reps} after {args.warmup} (min..max of the repetitions; spread = (max - min) / median), "
             f"kernel sources {source_sha16()}, {torch.cuda.get_device_name(0)}; ratio = row median / dense median",
             f"{'route':58s} {'median ms':>10s} {'min..max ms':>21s} {'spread':>7s} {'ratio':>7s}"]
    print(lines[0])
    print(lines[1], flush=True)
    labels = ("dense: affine_phase_scores, 64 entries x 64 shifts inside", f"listed (parent route): affine_scores over {K * 64} candidates")
    ms = alternate((dense_call, listed_call), args.reps, args.warmup)
    med = [float(np.median(m)) for m in ms]
    for name, m, t in zip(labels, ms, med):
        lines.append(f"{name:58s} {t:10.3f} {m.min():10.3f}..{m.max():<10.3f} {100 * (m.max() - m.min()) / t:6.1f}% {t / med[0]:7.2f}")
        print(lines[-1], flush=True)
    if ms[0].max() < ms[1].min():
        how = "IS faster beyond the spread than"
    elif ms[1].max() < ms[0].min():
        how = "is SLOWER beyond the spread than"
    else:
        how = "is NOT beyond the spread of (medians " + ("faster" if med[0] < med[1] else "slower") + ")"
    tail = [f"the dense call {how} the listed route (dense {ms[0].min():.3f}..{ms[0].max():.3f} ms, median {med[0]:.3f}; listed "
            f"{ms[1].min():.3f}..{ms[1].max():.3f} ms, median {med[1]:.3f}; {med[0] / (K * 64) * 1e3:.2f} against {med[1] / (K * 64) * 1e3:.2f} us "
            f"per shifted geometry)"]
    assert torch.equal(dense.reshape(n, K * 64), listed)
    host_units = np.array([eng.affine_units((h, w), (H, W), g)[4] for g in shifted[::97]])
    assert np.array_equal(units.reshape(-1).cpu().numpy()[::97], host_units)
    tail.append("identical results: dense scores == listed scores for all 4096 geometries and 8 frames (asserted); units == ofmk_affine_units "
                "on every 97th geometry (asserted)")
    found = resync.best_shifted_geometry(dense.cpu().numpy(), units.cpu().numpy(), cands)
    nrm = found["normalised"]
    order = np.argsort(-nrm.max(axis=1), kind="stable")
    tail.append(f"search: true entry {true_k} (angle {ANGLE}, sub-pixel shift {true_sub}, expected phase {true_phase}, {residual:.3f} px from the "
                f"lattice); found entry {found['index']} at phase {found['phase']}; the true entry's rank among the {K} entries is "
                f"{int(np.flatnonzero(order == true_k)[0]) + 1}; normalised {nrm.max():.4f} at the best shifted geometry "
                f"({int(units[found['index'], 8 * found['phase'][0] + found['phase'][1]])} units) against {np.delete(nrm, found['index'], axis=0).max():.4f} "
                f"best other entry (contrast {found['contrast']:.3f}) and {np.sort(nrm[found['index']])[-2]:.4f} second-best phase of the same "
                f"entry (phase contrast {found['phase_contrast']:.3f})")
    cand_payloads = [[payload_for_segment(s + 1, c) for c in range(2)] for s in range(2)]
    got = resync.read_transformed_leak(DwtDctSvdDecoder(), leak, seg, (H, W), cand_payloads, cands, key=0, L=L, search_frames=n)
    tail.append(f"read_transformed_leak: entry {got['index']} phase {got['phase']} copies {[int(p) for p in got['picks']]} (marked: {list(CHOSEN)}), "
                f"base {got['base']}, score {got['score']} against {got['runner_up_score']} for the best other base, ambiguous {got['ambiguous']}")
    lines += tail
    for ln in tail:
        print(ln)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
