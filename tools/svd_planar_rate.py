"""DwtDctSvd on 4:2:0 planes: the chain (yuv420_to_rgb -> svd_* on u8 RGB -> rgb_to_yuv420) against the fused
ofmk_svd_*_yuv420 calls, 300 x 1080p, I420 and NV12, blk 4 and 8, default scales [0, 15, 0].

Per step (embed, detect, embed + verify): ms per call (mean of --reps after --warmup), frames/s, and the fraction of 8 TB/s
that the step's ALGORITHMIC bytes per pixel represent (chain 15 / 7.5 / 22.5 B/px, fused 3 / 1.5 / 3 B/px).  The fused calls
are timed with dispatch events (an ofmk_timing object, kind "svd": the kernel's own begin / end timestamps); the chain's
conversion kernels carry no events, so the chain is timed with stream events around its three calls, and the fused call is
timed the same way too, for a like-for-like column.  The RGB kernel alone (svd on u8 RGB, dispatch events) is the reference
for the question the last column answers: a fused kernel far below the memory roofline (< 0.5 of 8 TB/s on its bytes) that takes
about as long as the RGB kernel of the same step, which moves twice the bytes, is bound by its arithmetic (VALU).
usage: python tools/svd_planar_rate.py [--frames 300] [--reps 5] [--warmup 2] [--out FILE]"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-fingerprinting_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from offmark import _hip  # noqa: E402
from offmark.engine import DctEngine  # noqa: E402
from offmark.generator.shuffler import Shuffler  # noqa: E402
from offmark.synthetic import synthetic_frames  # noqa: E402

SPEC_BPS = 8.0e12
BPX = {"embed": (15.0, 3.0), "detect": (7.5, 1.5), "embed_detect": (22.5, 3.0)}     # (chain, fused) algorithmic B/px
L = 8


def source_sha16():
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "video-fingerprinting_amd", "csrc")
    for path in sorted(os.path.join(csrc, f) for f in os.listdir(csrc)) + [os.path.join(ROOT, "include", "offmark_hip.h")]:
        h.update(os.path.basename(path).encode() + b"\0" + open(path, "rb").read())
    return h.hexdigest()[:16]


def stream_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def dispatch_ms(fn, reps, warmup):
    """Mean per call of the "svd" dispatch durations (ofmk_timing), and launches per call."""
    for _ in range(warmup):
        fn(None)
    torch.cuda.synchronize()
    tm = _hip.Timing(64 * reps)
    o = tm.opts()
    for _ in range(reps):
        fn(o)
    torch.cuda.synchronize()
    got = tm.collect()["svd"]
    tm.close()
    return got["ms_total"] / reps, got["launches"] / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, H, W = args.frames, 1080, 1920
    torch.cuda.set_device(0)
    eng = DctEngine()
    rgb = synthetic_frames(n, H, W, seed=2000)
    wm = torch.from_numpy(Shuffler(key=0).generate_wm(np.array([0, 1, 1, 0, 0, 1, 0, 1]), (1, H * W // 64)).astype(np.uint8)).cuda()
    rgb_out = torch.empty_like(rgb)
    lines = [f"# tools/svd_planar_rate.py: {n} x {H}x{W}, scales [0, 15, 0], kernel sources {source_sha16()}, "
             f"{torch.cuda.get_device_name(0)}; fraction = algorithmic B/px x pixels / time / 8 TB/s",
             f"{'layout':6s} {'blk':>3s} {'step':12s} {'chain ms':>9s} {'fused ms':>9s} {'fused(ev)':>9s} {'launch':>6s} {'rgb ms':>8s} "
             f"{'speedup':>7s} {'fused fps':>10s} {'chain frac':>10s} {'fused frac':>10s}  fused / RGB kernel, bound"]
    px = float(n) * H * W
    for layout in ("i420", "nv12"):
        planes = eng.rgb_to_yuv420(rgb, layout)
        out = torch.empty_like(planes)
        for blk in (4, 8):
            def chain(step):
                def go():
                    r = eng.yuv420_to_rgb(planes, H, W, layout)
                    if step == "detect":
                        eng.svd_detect(r, L, blk=blk)
                        return
                    eng.rgb_to_yuv420(eng.svd_embed(r, wm, blk=blk, out=rgb_out), layout, out=out)
                    if step == "embed_detect":                           # the chain's verify: its detect of the written planes
                        eng.svd_detect(eng.yuv420_to_rgb(out, H, W, layout), L, blk=blk)
                return go

            def fused(step, e=eng):
                if step == "embed":
                    return lambda: e.svd_embed_yuv420(planes, H, W, wm, blk=blk, out=out, layout=layout)
                if step == "detect":
                    return lambda: e.svd_detect_yuv420(planes, H, W, L, blk=blk, layout=layout)
                return lambda: e.svd_embed_detect_yuv420(planes, H, W, wm, L, blk=blk, out=out, layout=layout)

            def with_opts(step, kind):
                def go(o):
                    e = DctEngine(opts=o) if o is not None else eng
                    if kind == "fused":
                        fused(step, e)()
                    elif step == "detect":
                        e.svd_detect(rgb, L, blk=blk)
                    elif step == "embed":
                        e.svd_embed(rgb, wm, blk=blk, out=rgb_out)
                    else:
                        e.svd_embed_detect(rgb, wm, L, blk=blk, out=rgb_out)
                return go

            for step in ("embed", "detect", "embed_detect"):
                c_ms = stream_ms(chain(step), args.reps, args.warmup)
                f_ev = stream_ms(fused(step), args.reps, args.warmup)
                f_ms, launches = dispatch_ms(with_opts(step, "fused"), args.reps, args.warmup)
                r_ms, _ = dispatch_ms(with_opts(step, "rgb"), args.reps, args.warmup)
                cb, fb = BPX[step]
                c_frac = cb * px / (c_ms * 1e-3) / SPEC_BPS
                f_frac = fb * px / (f_ms * 1e-3) / SPEC_BPS
                bound = f"{f_ms / r_ms:.2f} x RGB kernel, " + ("memory-bound" if f_frac >= 0.5 else "VALU-bound")
                lines.append(f"{layout:6s} {blk:3d} {step:12s} {c_ms:9.3f} {f_ms:9.3f} {f_ev:9.3f} {launches:6.1f} {r_ms:8.3f} "
                             f"{c_ms / f_ev:7.2f} {n / (f_ms * 1e-3):10.0f} {c_frac:10.3f} {f_frac:10.3f}  {bound}")
                print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(lines[0])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
