"""C marked AND verified copies of the same frames with the DCT codec, 300 x 1080p, C in {2, 3, 8}, L = 8: three routes to the
same [C, n, H, W, 3] copies and [C, n, L] counts --
  fused : embed_detect_copies (ofmk_embed_detect_copies_rgb8): every copy is read out from the pixels the mark kernel holds
  chain : embed_copies, then detect of every written copy -- what fingerprint.mark_segment_copies did before the fused call
          existed; the BASELINE of the speed-up column
  loop  : embed_detect once per copy (the single-copy fused mark + verify)

The routes are timed one after the other in every repetition, in the same process (stream events around one route), mean of
--reps after --warmup, with the spread (min..max) of each route's repetitions next to its mean.  Per row: ms, frames x copies per
second, the route's ALGORITHMIC bytes per pixel (fused 6 + 3C, chain 6 + 6C, loop 9C) as a fraction of 8 TB/s, and the modelled
speed-up over the chain, (6 + 6C) / (6 + 3C), beside the measured one.  All three routes' copies and counts are asserted identical.
usage: python tools/copies_verify_rate.py [--frames 300] [--reps 5] [--warmup 2] [--copies 2 3 8] [--out FILE]"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-fingerprinting_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from offmark.engine import DctEngine  # noqa: E402
from offmark.fingerprint import payload_for_segment  # noqa: E402
from offmark.generator.shuffler import Shuffler  # noqa: E402
from offmark.synthetic import synthetic_frames  # noqa: E402

SPEC_BPS = 8.0e12
L = 8


def source_sha16():
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "video-fingerprinting_amd", "csrc")
    for path in sorted(os.path.join(csrc, f) for f in os.listdir(csrc)) + [os.path.join(ROOT, "include", "offmark_hip.h")]:
        h.update(os.path.basename(path).encode() + b"\0" + open(path, "rb").read())
    return h.hexdigest()[:16]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(routes, reps, warmup):
    """ms of every repetition of each route, the routes timed one after the other in every repetition."""
    for _ in range(warmup):
        for fn in routes:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in routes]
    for _ in range(reps):
        for k, fn in enumerate(routes):
            ms[k].append(timed(fn))
    return [np.asarray(m) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--copies", type=int, nargs="+", default=[2, 3, 8])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, H, W = args.frames, 1080, 1920
    torch.cuda.set_device(0)
    eng = DctEngine()
    frames = synthetic_frames(n, H, W, seed=2000)
    cmax = max(args.copies)
    gen = Shuffler(key=0)
    wm = torch.from_numpy(np.stack([gen.generate_wm(payload_for_segment(1, c), (H * W // 64,)) for c in range(cmax)])
                          .astype(np.uint8)).cuda()
    lines = [f"# tools/copies_verify_rate.py: {n} x {H}x{W}, DCT copies + verify (L = {L}): fused call vs chain (embed_copies, then detect "
             f"of each copy; the baseline) vs per-copy embed_detect loop; routes alternating, mean of {args.reps} after {args.warmup} "
             f"(min..max of the repetitions), kernel sources {source_sha16()}, {torch.cuda.get_device_name(0)}; "
             f"frac = algorithmic B/px x pixels / time / 8 TB/s; speedup = chain ms / route ms, model = (6 + 6C) / route B/px",
             f"{'route':6s} {'C':>2s} {'ms':>9s} {'min..max ms':>19s} {'fps x C':>9s} {'B/px':>5s} {'frac':>6s} {'speedup':>7s} {'model':>6s}"]
    print(lines[0])
    print(lines[1], flush=True)
    px = float(n) * H * W
    verdicts = []
    for C in args.copies:
        rows = torch.arange(C, dtype=torch.int32, device="cuda")[:, None].repeat(1, n).contiguous()
        outs = [torch.empty((C, n, H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(3)]
        cnts = [torch.empty((C, n, L), dtype=torch.int32, device="cuda") for _ in range(3)]

        def fused():
            eng.embed_detect_copies(frames, wm, rows, L, out=outs[0], counts=cnts[0])

        def chain():
            eng.embed_copies(frames, wm, rows, out=outs[1])
            for c in range(C):
                eng.detect(outs[1][c], L, counts=cnts[1][c])

        def loop():
            for c in range(C):
                eng.embed_detect(frames, wm, L, wm_row=rows[c], out=outs[2][c], counts=cnts[2][c])
        ms = alternate((fused, chain, loop), args.reps, args.warmup)
        for k in (1, 2):
            assert torch.equal(outs[0], outs[k]) and torch.equal(cnts[0], cnts[k]), (C, k)
        bpx = (6.0 + 3.0 * C, 6.0 + 6.0 * C, 9.0 * C)
        t_chain = float(ms[1].mean())
        for name, m, b in zip(("fused", "chain", "loop"), ms, bpx):
            t = float(m.mean())
            lines.append(f"{name:6s} {C:2d} {t:9.3f} {m.min():9.3f}..{m.max():<9.3f} {n * C / (t * 1e-3):9.0f} {b:5.0f} "
                         f"{b * px / (t * 1e-3) / SPEC_BPS:6.3f} {t_chain / t:7.2f} {bpx[1] / b:6.2f}")
            print(lines[-1], flush=True)
        # faster by more than the repetitions' own spread: the slowest fused repetition beats the fastest chain repetition
        verdicts.append(f"C = {C}: fused {'IS' if ms[0].max() < ms[1].min() else 'is NOT'} faster than the chain beyond the spread "
                        f"(slowest fused {ms[0].max():.3f} ms, fastest chain {ms[1].min():.3f} ms)")
        del outs, cnts
        torch.cuda.empty_cache()
    lines += verdicts
    lines.append("identical copies and counts on all three routes: yes (asserted for every C)")
    for ln in lines[-len(verdicts) - 1:]:
        print(ln)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
