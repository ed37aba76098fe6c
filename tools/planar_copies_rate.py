"""C marked copies of the same 4:2:0 frames: the one-pass calls (ofmk_embed_copies_yuv420, ofmk_svd_embed_copies_yuv420) against
the per-copy loop of the single-copy planar calls, 300 x 1080p, I420 and NV12, C in {2, 3, 8}: DCT embed, DwtDctSvd (blk 4,
scales [0, 15, 0]) embed and embed + verify.  For --chain-copies (default 3) also against the chain through the RGB copies
kernels: yuv420_to_rgb, *_copies_rgb8, rgb_to_yuv420 of every copy.

The routes are timed alternately in the same process (stream events around one call, or around the calls of the loop / the
chain), --reps after --warmup.  Per row: mean ms of each route, the loop's spread (max - min of its repetitions; the one-pass
call has to win by more than that), the speedup next to the model's, frames x copies per second, the one-pass route's
ALGORITHMIC bytes per pixel (1.5 + 1.5 C; the DCT codec's analyze reads 1.5 more) as a fraction of 8 TB/s, and which bound that
suggests (below 0.5: limited by its arithmetic, VALU, not by HBM).  Model: DCT = the loop pays analyze C times, one pass once,
with analyze : mark = 0.35 : 0.875 ms and the per-copy marking cost unchanged; DwtDctSvd = ratio of the
algorithmic bytes, 3 C / (1.5 + 1.5 C).  All routes' outputs (and the verify's counts) are asserted identical.
usage: python tools/planar_copies_rate.py [--frames 300] [--reps 5] [--warmup 2] [--copies 2 3 8] [--layouts i420 nv12] [--out FILE]"""
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
T_ANALYZE, T_MARK = 0.35, 0.875          # ms per 300 x 1080p of the planar analyze and non-fused mark kernels


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
    """ms of every route per repetition, the routes timed one after the other in every repetition."""
    for _ in range(warmup):
        for fn in routes:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in routes]
    for _ in range(reps):
        for i, fn in enumerate(routes):
            ms[i].append(timed(fn))
    return [np.asarray(m) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--copies", type=int, nargs="+", default=[2, 3, 8])
    ap.add_argument("--chain-copies", type=int, default=3)
    ap.add_argument("--layouts", nargs="+", default=["i420", "nv12"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, H, W = args.frames, 1080, 1920
    fb = H * W * 3 // 2
    torch.cuda.set_device(0)
    eng = DctEngine()
    rgb_src = synthetic_frames(n, H, W, seed=2000)
    cmax = max(args.copies)
    gen = Shuffler(key=0)
    wm = torch.from_numpy(np.stack([gen.generate_wm(payload_for_segment(1, c), (H * W // 64,)) for c in range(cmax)])
                          .astype(np.uint8)).cuda()
    lines = [f"# tools/planar_copies_rate.py: {n} x {H}x{W} 4:2:0, one pass vs per-copy loop vs RGB-copies chain (alternating, "
             f"{args.reps} reps after {args.warmup}), kernel sources {source_sha16()}, {torch.cuda.get_device_name(0)}; "
             f"frac = algorithmic B/px x pixels / time / 8 TB/s; spread = max - min of the loop's repetitions",
             f"{'layout':6s} {'codec':5s} {'step':12s} {'C':>2s} {'loop ms':>8s} {'spread':>6s} {'1-pass ms':>9s} {'speedup':>7s} {'model':>5s} "
             f"{'beats loop':>10s} {'chain ms':>8s} {'vs chain':>8s} {'loop fps':>9s} {'1-pass fps':>10s} {'1p B/px':>7s} {'1p frac':>7s}  bound (1 pass)"]
    print(lines[0])
    print(lines[1], flush=True)
    px = float(n) * H * W
    for layout in args.layouts:
        planes = eng.rgb_to_yuv420(rgb_src, layout)
        for codec, step in (("dct", "embed"), ("svd", "embed"), ("svd", "embed_verify")):
            for C in args.copies:
                rows = torch.arange(C, dtype=torch.int32, device="cuda")[:, None].repeat(1, n).contiguous()
                out_one = torch.empty((C, n, fb), dtype=torch.uint8, device="cuda")
                out_loop = torch.empty_like(out_one)
                cnt_one = torch.empty((C, n, L), dtype=torch.int32, device="cuda")
                cnt_loop = torch.empty_like(cnt_one)
                chain = C == args.chain_copies
                if chain:
                    rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
                    rgb_out = torch.empty((C, n, H, W, 3), dtype=torch.uint8, device="cuda")
                    out_chain = torch.empty_like(out_one)
                if codec == "dct":
                    def one():
                        eng.embed_copies_yuv420(planes, H, W, wm, rows, out=out_one, layout=layout)

                    def loop():
                        for c in range(C):
                            eng.embed_yuv420(planes, H, W, wm, wm_row=rows[c], out=out_loop[c], layout=layout)

                    def rgb_copies():
                        eng.embed_copies(rgb, wm, rows, out=rgb_out)
                    one_bpx = 3.0 + 1.5 * C
                    model = C * (T_ANALYZE + T_MARK) / (T_ANALYZE + C * T_MARK)
                elif step == "embed":
                    def one():
                        eng.svd_embed_copies_yuv420(planes, H, W, wm, rows, out=out_one, layout=layout)

                    def loop():
                        for c in range(C):
                            eng.svd_embed_yuv420(planes, H, W, wm, wm_row=rows[c], out=out_loop[c], layout=layout)

                    def rgb_copies():
                        eng.svd_embed_copies(rgb, wm, rows, out=rgb_out)
                    one_bpx = 1.5 + 1.5 * C
                    model = 3.0 * C / one_bpx
                else:
                    def one():
                        eng.svd_embed_copies_yuv420(planes, H, W, wm, rows, out=out_one, L=L, counts=cnt_one, layout=layout)

                    def loop():
                        for c in range(C):
                            eng.svd_embed_detect_yuv420(planes, H, W, wm, L, wm_row=rows[c], out=out_loop[c], counts=cnt_loop[c],
                                                        layout=layout)

                    def rgb_copies():
                        eng.svd_embed_copies(rgb, wm, rows, out=rgb_out)      # the chain's verify would read the planes again: not timed
                    one_bpx = 1.5 + 1.5 * C
                    model = 3.0 * C / one_bpx

                def chain_route():
                    eng.yuv420_to_rgb(planes, H, W, layout, out=rgb)
                    rgb_copies()
                    for c in range(C):
                        eng.rgb_to_yuv420(rgb_out[c], layout, out=out_chain[c])
                ms = alternate([one, loop] + ([chain_route] if chain else []), args.reps, args.warmup)
                assert torch.equal(out_one, out_loop), (layout, codec, step, C)
                if step == "embed_verify":
                    assert torch.equal(cnt_one, cnt_loop), (layout, codec, step, C)
                if chain:
                    assert torch.equal(out_one, out_chain), (layout, codec, step, C, "chain")
                t_one, t_loop = float(ms[0].mean()), float(ms[1].mean())
                spread = float(ms[1].max() - ms[1].min())
                t_chain = float(ms[2].mean()) if chain else float("nan")
                f_one = one_bpx * px / (t_one * 1e-3) / SPEC_BPS
                bound = "memory-bound" if f_one >= 0.5 else "VALU-bound"
                beats = "yes" if t_loop - t_one > spread else "NO"
                lines.append(f"{layout:6s} {codec:5s} {step:12s} {C:2d} {t_loop:8.3f} {spread:6.3f} {t_one:9.3f} {t_loop / t_one:7.2f} {model:5.2f} "
                             f"{beats:>10s} {t_chain:8.3f} {t_chain / t_one:8.2f} {n * C / (t_loop * 1e-3):9.0f} {n * C / (t_one * 1e-3):10.0f} "
                             f"{one_bpx:7.1f} {f_one:7.3f}  {bound}")
                print(lines[-1], flush=True)
                del out_one, out_loop
                if chain:
                    del rgb, rgb_out, out_chain
                torch.cuda.empty_cache()
        del planes
    print("identical outputs: yes (asserted for every row)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\nidentical outputs: yes (asserted for every row)\n")


if __name__ == "__main__":
    main()
