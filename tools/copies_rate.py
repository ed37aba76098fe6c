"""C marked copies of the same frames: the one-pass calls (ofmk_embed_copies_rgb8, ofmk_svd_embed_copies_rgb8) against the
per-copy loop of the single-copy calls, 300 x 1080p, C in {2, 3, 8}: DCT embed, DwtDctSvd (blk 4, scales [0, 15, 0]) embed and
embed + verify.

The two routes are timed alternately in the same process (stream events around one call, or around the C calls of the loop),
mean of --reps after --warmup.  Per row: ms, frames x copies per second, the route's ALGORITHMIC bytes per pixel (DCT: loop 9C,
one pass 6 + 3C; DwtDctSvd: loop 6C, one pass 3 + 3C; the verify reads nothing more) as a fraction of 8 TB/s, and which bound
that suggests (a fraction below 0.5 means the kernel is limited by its arithmetic, VALU, not by HBM).  Both routes' outputs
(and the verify's counts) are asserted identical.
usage: python tools/copies_rate.py [--frames 300] [--reps 5] [--warmup 2] [--copies 2 3 8] [--out FILE]"""
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


def alternate(one, loop, reps, warmup):
    """Mean ms of each route, timed one after the other in every repetition."""
    for _ in range(warmup):
        one()
        loop()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(reps):
        a.append(timed(one))
        b.append(timed(loop))
    return float(np.mean(a)), float(np.mean(b))


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
    lines = [f"# tools/copies_rate.py: {n} x {H}x{W}, one pass vs per-copy loop (alternating, mean of {args.reps} after "
             f"{args.warmup}), kernel sources {source_sha16()}, {torch.cuda.get_device_name(0)}; "
             f"frac = algorithmic B/px x pixels / time / 8 TB/s",
             f"{'codec':8s} {'step':12s} {'C':>2s} {'loop ms':>9s} {'1-pass ms':>9s} {'speedup':>7s} {'model':>6s} "
             f"{'loop fps':>9s} {'1-pass fps':>10s} {'loop B/px':>9s} {'1p B/px':>7s} {'loop frac':>9s} {'1p frac':>7s}  bound (1 pass)"]
    print(lines[0])
    print(lines[1], flush=True)
    px = float(n) * H * W
    for codec, step in (("dct", "embed"), ("svd", "embed"), ("svd", "embed_verify")):
        for C in args.copies:
            rows = torch.arange(C, dtype=torch.int32, device="cuda")[:, None].repeat(1, n).contiguous()
            out_one = torch.empty((C, n, H, W, 3), dtype=torch.uint8, device="cuda")
            out_loop = torch.empty_like(out_one)
            cnt_one = torch.empty((C, n, L), dtype=torch.int32, device="cuda")
            cnt_loop = torch.empty_like(cnt_one)
            if codec == "dct":
                def one():
                    eng.embed_copies(frames, wm, rows, out=out_one)

                def loop():
                    for c in range(C):
                        eng.embed(frames, wm, wm_row=rows[c], out=out_loop[c])
                loop_bpx, one_bpx = 9.0 * C, 6.0 + 3.0 * C
            elif step == "embed":
                def one():
                    eng.svd_embed_copies(frames, wm, rows, out=out_one)

                def loop():
                    for c in range(C):
                        eng.svd_embed(frames, wm, wm_row=rows[c], out=out_loop[c])
                loop_bpx, one_bpx = 6.0 * C, 3.0 + 3.0 * C
            else:
                def one():
                    eng.svd_embed_copies(frames, wm, rows, out=out_one, L=L, counts=cnt_one)

                def loop():
                    for c in range(C):
                        eng.svd_embed_detect(frames, wm, L, wm_row=rows[c], out=out_loop[c], counts=cnt_loop[c])
                loop_bpx, one_bpx = 6.0 * C, 3.0 + 3.0 * C
            t_one, t_loop = alternate(one, loop, args.reps, args.warmup)
            assert torch.equal(out_one, out_loop), (codec, step, C)
            if step == "embed_verify":
                assert torch.equal(cnt_one, cnt_loop), (codec, step, C)
            f_loop = loop_bpx * px / (t_loop * 1e-3) / SPEC_BPS
            f_one = one_bpx * px / (t_one * 1e-3) / SPEC_BPS
            bound = "memory-bound" if f_one >= 0.5 else "VALU-bound"
            lines.append(f"{codec:8s} {step:12s} {C:2d} {t_loop:9.3f} {t_one:9.3f} {t_loop / t_one:7.2f} {loop_bpx / one_bpx:6.2f} "
                         f"{n * C / (t_loop * 1e-3):9.0f} {n * C / (t_one * 1e-3):10.0f} {loop_bpx:9.0f} {one_bpx:7.0f} "
                         f"{f_loop:9.3f} {f_one:7.3f}  {bound}")
            print(lines[-1], flush=True)
            del out_one, out_loop
            torch.cuda.empty_cache()
    print("identical outputs: yes (asserted for every row)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
