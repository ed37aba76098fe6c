"""C marked and verified copies WITH the soft sums of every copy, 300 x 1080p, C in {2, 3, 8}, L = 8, both codecs on RGB and DwtDctSvd
(blk 4) on I420 planes: two routes to the same copies, counts and int64 [C, n, L] soft sums --
  fused    : the copies call with ``soft=`` (ofmk_*_copies_soft_*): the soft sums come from the pixels / records the copies kernels hold
  sequence : the copies-with-verify call as it was, then the stand-alone soft read-out of every written copy (3 C B/px more on RGB,
             1.5 C on planes); the BASELINE

The two routes alternate call by call in one process (stream events around one call); per row the median of --reps calls after
--warmup, the spread (min..max) of the repetitions, and the sequence's median over the route's.  Both routes' results are asserted
identical.  The verdict per codec and C says whether the fused route is faster beyond the spread: its slowest call beats the
sequence's fastest.
usage: python tools/copies_soft_rate.py [--frames 300] [--reps 30] [--warmup 3] [--copies 2 3 8] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-fingerprinting_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from copies_verify_rate import alternate, source_sha16  # noqa: E402
from offmark.engine import DctEngine  # noqa: E402
from offmark.fingerprint import payload_for_segment  # noqa: E402
from offmark.generator.shuffler import Shuffler  # noqa: E402
from offmark.synthetic import synthetic_frames  # noqa: E402

L = 8


def routes_of(codec, eng, src, H, W, wm, rows, C, n):
    """(fused, sequence, results): the two routes as callables writing into their own buffers, and those buffers per route."""
    dev = src.device
    shape = (C, n, H * W * 3 // 2) if codec == "svd_i420" else (C, n, H, W, 3)
    res = [dict(out=torch.empty(shape, dtype=torch.uint8, device=dev), counts=torch.empty((C, n, L), dtype=torch.int32, device=dev),
                soft=torch.empty((C, n, L), dtype=torch.int64, device=dev)) for _ in range(2)]
    if codec == "dct_rgb":
        def fused():
            eng.embed_detect_copies(src, wm, rows, L, **res[0])

        def sequence():
            eng.embed_detect_copies(src, wm, rows, L, out=res[1]["out"], counts=res[1]["counts"])
            for c in range(C):
                eng.detect_soft(res[1]["out"][c], L, soft=res[1]["soft"][c])
    elif codec == "svd_rgb":
        def fused():
            eng.svd_embed_copies(src, wm, rows, L=L, **res[0])

        def sequence():
            eng.svd_embed_copies(src, wm, rows, L=L, out=res[1]["out"], counts=res[1]["counts"])
            for c in range(C):
                eng.svd_detect_soft(res[1]["out"][c], L, soft=res[1]["soft"][c])
    else:
        def fused():
            eng.svd_embed_copies_yuv420(src, H, W, wm, rows, L=L, **res[0])

        def sequence():
            eng.svd_embed_copies_yuv420(src, H, W, wm, rows, L=L, out=res[1]["out"], counts=res[1]["counts"])
            for c in range(C):
                eng.svd_detect_soft_yuv420(res[1]["out"][c], H, W, L, soft=res[1]["soft"][c])
    return fused, sequence, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--copies", type=int, nargs="+", default=[2, 3, 8])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, H, W = args.frames, 1080, 1920
    torch.cuda.set_device(0)
    eng = DctEngine()
    frames = synthetic_frames(n, H, W, seed=2000)
    planes = eng.rgb_to_yuv420(frames, "i420")
    gen = Shuffler(key=0)
    wm = torch.from_numpy(np.stack([gen.generate_wm(payload_for_segment(1, c), (H * W // 64,)) for c in range(max(args.copies))])
                          .astype(np.uint8)).cuda()
    lines = [f"# tools/copies_soft_rate.py: {n} x {H}x{W}, copies + verify + soft sums (L = {L}): the copies call with soft= (fused) vs the "
             f"copies-with-verify call followed by the soft read-out of each copy (sequence; the baseline); routes alternating call by "
             f"call, median of {args.reps} after {args.warmup} (min..max of the repetitions; spread = (max - min) / median), kernel "
             f"sources {source_sha16()}, {torch.cuda.get_device_name(0)}; speedup = sequence median / route median",
             f"{'codec':9s} {'route':8s} {'C':>2s} {'median ms':>10s} {'min..max ms':>19s} {'spread':>7s} {'fps x C':>9s} {'speedup':>7s}"]
    print(lines[0])
    print(lines[1], flush=True)
    verdicts = []
    for codec in ("dct_rgb", "svd_rgb", "svd_i420"):
        src = planes if codec == "svd_i420" else frames
        for C in args.copies:
            rows = torch.arange(C, dtype=torch.int32, device="cuda")[:, None].repeat(1, n).contiguous()
            fused, sequence, res = routes_of(codec, eng, src, H, W, wm, rows, C, n)
            ms = alternate((fused, sequence), args.reps, args.warmup)
            assert all(torch.equal(res[0][k], res[1][k]) for k in ("out", "counts", "soft")), (codec, C)
            med = [float(np.median(m)) for m in ms]
            for name, m, t in zip(("fused", "sequence"), ms, med):
                lines.append(f"{codec:9s} {name:8s} {C:2d} {t:10.3f} {m.min():9.3f}..{m.max():<9.3f} {100 * (m.max() - m.min()) / t:6.1f}% "
                             f"{n * C / (t * 1e-3):9.0f} {med[1] / t:7.2f}")
                print(lines[-1], flush=True)
            verdicts.append(f"{codec} C = {C}: fused {'IS' if ms[0].max() < ms[1].min() else 'is NOT'} faster than the sequence beyond the "
                            f"spread (slowest fused {ms[0].max():.3f} ms, fastest sequence {ms[1].min():.3f} ms; medians {med[0]:.3f} / {med[1]:.3f})")
            del res, fused, sequence
            torch.cuda.empty_cache()
    lines += verdicts
    lines.append("identical copies, counts and soft sums on both routes: yes (asserted for every codec and C)")
    for ln in lines[-len(verdicts) - 1:]:
        print(ln)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
