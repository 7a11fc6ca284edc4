"""Progressive frames (rt_accumulate_samples_device + rt_resolve_device) next to the composition
that made the same frame before them, and to rt_render_device.

Per config (default c2 at 1920x1080 with aa_samples = 4, and C1's own 1000x1000 at aa_samples =
32, the reference main()'s), one frame's float64 pixels three ways, all on one stream:
  (a) fused      accumulate_device(0, N) + resolve_device: two launches
      fused_acc  accumulate_device(0, N) alone, and fused_acc1 accumulate_device(0, 1): the
                 per-sample cost of the sum is (t(0, N) - t(0, 1)) / (N - 1)
  (b) composed   the parent's composition: per sample camera_rays_device + trace_rays_device + a
                 torch add into the sum (3 N launches, 144 B of rays, colours and sum through HBM
                 per pixel and sample more than (a)), then a torch divide; composed_1 is one
                 sample's three launches (sample 1: a jittered one)
  (c) render     rt_render_device, for information: the packet / box / breadth-first kernels the
                 sample ranges are not routed through
HIP events around `--launches` back-to-back frames on the context's stream, per frame, the routes
alternating inside one process after a warm-up of each; median and min .. max of `--repeats`
repeats.  Before timing, the three frames are compared bit for bit at the timed size.

  python tools/accumulate_time.py [--configs c2:1920x1080:4,c1:1000x1000:32]
                                  [--out profiles/accumulate_time.txt]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2:1920x1080:4,c1:1000x1000:32")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from raytracingengine_amd import capi
    from raytracingengine_amd.configs import make_config

    lines = ["# accumulate_device(0, N) + resolve_device (fused) next to the per-sample composition",
             "# camera_rays_device + trace_rays_device + torch add, then a torch divide (composed), and",
             "# to rt_render_device; one MI355X; us per frame (median of the repeats, min .. max), HIP",
             "# events around back-to-back frames on one stream; see tools/accumulate_time.py.",
             f"# build {capi.build_info()['source_sha256'][:16]}, {args.launches} frames per repeat, "
             f"{args.repeats} repeats"]
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)

    def frame_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.launches):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.launches

    def measure(routes):
        for fn in routes.values():
            fn()
        ctx.synchronize()
        t_end = time.perf_counter() + 0.3   # warm-up past the clock ramp
        while time.perf_counter() < t_end:
            for fn in routes.values():
                frame_us(fn)
        reps = {k: [] for k in routes}
        for _ in range(args.repeats):
            for k, fn in routes.items():
                reps[k].append(frame_us(fn))
        ctx.synchronize()
        return reps

    verdicts = []
    for spec in args.configs.split(","):
        name, size, aa = spec.split(":")
        W, H = (int(v) for v in size.split("x"))
        N = int(aa)
        sc = make_config(name, W, H, N)
        ds = ctx.scene(sc)
        px = W * H
        o = capi.default_opts()
        with torch.cuda.stream(stream):
            d_sum = torch.empty((px, 3), dtype=torch.float64, device="cuda")
            d_fused = torch.empty((px, 3), dtype=torch.float64, device="cuda")
            d_rays = torch.empty((px, 6), dtype=torch.float64, device="cuda")
            d_rgb = torch.empty((px, 3), dtype=torch.float64, device="cuda")
            d_acc = torch.empty((px, 3), dtype=torch.float64, device="cuda")
            d_comp = torch.empty((px, 3), dtype=torch.float64, device="cuda")
            d_frame = torch.empty((px, 3), dtype=torch.float64, device="cuda")
        stream.synchronize()

        def fused():
            ds.accumulate_device(0, N, sum=d_sum)
            ds.resolve_device(d_sum, N, out={"hdr64": d_fused})

        def one_sample(s):
            ds.camera_rays_device(s, out=d_rays)
            ds.trace_rays_device(d_rays, out=d_rgb)
            with torch.cuda.stream(stream):
                d_acc.add_(d_rgb)

        def composed():
            with torch.cuda.stream(stream):
                d_acc.zero_()
            for s in range(N):
                one_sample(s)
            with torch.cuda.stream(stream):
                torch.div(d_acc, float(N), out=d_comp)

        def render():
            ds.render_device(d_frame.data_ptr(), None, None, o)

        # the three frames at the timed size, as bits
        fused()
        composed()
        render()
        ctx.synchronize()
        eq_comp = bool(torch.equal(d_fused.view(torch.int64), d_comp.view(torch.int64)))
        eq_rend = bool(torch.equal(d_fused.view(torch.int64), d_frame.view(torch.int64)))
        routes = {"fused": fused, "composed": composed, "render": render,
                  "fused_acc": lambda: ds.accumulate_device(0, N, sum=d_sum),
                  "fused_acc1": lambda: ds.accumulate_device(0, 1, sum=d_sum),
                  "composed_1": lambda: one_sample(min(1, N - 1))}
        reps = measure(routes)
        med = {k: float(np.median(v)) for k, v in reps.items()}
        lines += ["", f"## {name} {W}x{H}, aa_samples = {N}: fused == composed: {eq_comp}, "
                      f"fused == rt_render_device: {eq_rend} (bit for bit, {px} pixels)"]
        for k, v in reps.items():
            lines.append(f"{k:12s} {np.median(v):11.1f} us   ({min(v):.1f} .. {max(v):.1f})")
        per_a = (med["fused_acc"] - med["fused_acc1"]) / (N - 1) if N > 1 else med["fused_acc"]
        lines.append(f"per sample:  fused {per_a:.1f} us = (t(0,{N}) - t(0,1)) / {max(N - 1, 1)}, "
                     f"composed {med['composed_1']:.1f} us (camera rays + trace + add of sample 1)")
        print("\n".join(lines[-(len(reps) + 2):]), flush=True)
        verdicts.append(f"{name} {W}x{H} aa {N}: fused {med['fused']:.1f} us, composed "
                        f"{med['composed']:.1f} us (fused / composed = "
                        f"{med['fused'] / med['composed']:.3f}), rt_render_device "
                        f"{med['render']:.1f} us (fused / render = {med['fused'] / med['render']:.2f}); "
                        f"per sample {per_a:.1f} us fused, {med['composed_1']:.1f} us composed; "
                        f"bits equal: composed {eq_comp}, render {eq_rend}")
        ds.close()

    ctx.close()
    lines += ["", "## summary"] + verdicts
    print("\n".join(verdicts), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
