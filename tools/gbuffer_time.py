"""G-buffer pass against its baselines on one GPU: per-frame times of

  (a) render        rt_render_device, hdr64 + Reinhard bytes (27 B/px)      [baseline]
  (b) gb_depth_prim rt_gbuffer_device DEPTH|PRIM (16 B/px)
  (c) gb_all        rt_gbuffer_device, all five outputs (56 B/px)
  (d) ray_route     rt_intersect_rays over host-built rays of every pixel,
                    transfers included (48 B/px up, 72 B/px down)            [baseline]

for a scene at its BASELINE resolution (default C2, 1920x1080).  (b) and (c) run with both tile
shapes of the packet kernel (8x8 and 16x4 pixels per wave: the store-shape A/B) and (c) also on
the generic kernel.  (a)-(c) are HIP-event times per launch (RT_FLAG_TIME_KERNEL); (d) is host
wall clock around the synchronous call.  The variants alternate inside one process in chunks of
`--chunk` launches, after a warm-up of every variant; `--repeats` repeats give the spread.

  python tools/gbuffer_time.py [--config c2] [--frames 200] [--route-frames 10] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from raytracingengine_amd import capi
from raytracingengine_amd.configs import make_config

HBM_PEAK = 8.0e12      # B/s, spec (MI355X)
HBM_MEASURED = 6.29e12  # B/s, float4 copy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--route-frames", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    sc = make_config(args.config)
    W, H = sc.camera.width, sc.camera.height
    px = W * H
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    ds = ctx.scene(sc)
    hdr = torch.empty(px * 3, dtype=torch.float64, device="cuda")
    ldr = torch.empty(px * 3, dtype=torch.uint8, device="cuda")
    lay = capi.gbuffer_layout(capi.GB_ALL, W, H)
    gb = {n: torch.empty(int(np.prod(s)) * d.itemsize, dtype=torch.uint8, device="cuda")
          for n, (s, d) in lay.items()}
    ptrs = {n: t.data_ptr() for n, t in gb.items()}
    timed = capi.RT_FLAG_TIME_KERNEL
    o_render = capi.default_opts(tonemap=1, flags=timed)
    o_gb = capi.default_opts(flags=timed)
    o_gen = capi.default_opts(flags=timed | capi.RT_FLAG_GENERIC_KERNEL)

    def gbuf(outputs, tile, o):
        def run():
            os.environ["RTAMD_GB_TILE"] = tile  # read per launch
            ds.gbuffer_device(outputs, ptrs, opts=o)
        return run

    dp = capi.GB_DEPTH | capi.GB_PRIM
    variants = {
        "render": (lambda: ds.render_device(hdr.data_ptr(), None, ldr.data_ptr(), o_render), 27),
        "gb_depth_prim_8x8": (gbuf(dp, "8", o_gb), 16),
        "gb_depth_prim_16x4": (gbuf(dp, "16", o_gb), 16),
        "gb_all_8x8": (gbuf(capi.GB_ALL, "8", o_gb), 56),
        "gb_all_16x4": (gbuf(capi.GB_ALL, "16", o_gb), 56),
        "gb_all_generic": (gbuf(capi.GB_ALL, "16", o_gen), 56),
    }
    # (d): the rays of every pixel, built on the host once (Camera::getRay, unjittered)
    cam = np.array(sc.camera.position)
    xs = np.arange(W) - W / 2.0
    ys = H / 2.0 - np.arange(H)
    d = np.stack(np.broadcast_arrays(xs[None, :], ys[:, None], np.float64(sc.camera.focal)), -1)
    d = d + np.array([0.0, 0.0, cam[2]]) - cam
    d /= np.sqrt((d * d).sum(-1, keepdims=True))
    rays = np.concatenate([np.broadcast_to(cam, d.shape), d], -1).reshape(-1, 6)

    def route():
        t0 = time.perf_counter()
        ds.intersect_rays(rays)
        return (time.perf_counter() - t0) * 1e3

    # warm-up: every variant, past the clock ramp
    t_end = time.perf_counter() + 0.3
    while time.perf_counter() < t_end:
        for run, _ in variants.values():
            for _ in range(4):
                run()
        ctx.synchronize()
    route()

    repeats = []
    for _ in range(args.repeats):
        ms = {k: 0.0 for k in variants}
        n = {k: 0 for k in variants}
        for _ in range(-(-args.frames // args.chunk)):
            for k, (run, _) in variants.items():
                ctx.reset_stats()
                for _ in range(args.chunk):
                    run()
                st = ctx.stats()
                ms[k] += st.kernel_ms
                n[k] += st.launches
        rep = {k: ms[k] / n[k] * 1e3 for k in variants}
        rep["ray_route"] = float(np.mean([route() for _ in range(args.route_frames)])) * 1e3
        repeats.append(rep)

    result = {"config": args.config, "width": W, "height": H, "frames_per_variant": args.frames,
              "route_frames": args.route_frames, "chunk": args.chunk, "unit": "us per frame",
              "build": capi.build_info()["source_sha256"], "variants": {}}
    for k in list(variants) + ["ray_route"]:
        v = [r[k] for r in repeats]
        e = {"mean_us": float(np.mean(v)), "min_us": min(v), "max_us": max(v), "repeats_us": v}
        if k in variants:
            b = variants[k][1] * px
            e["bytes_per_px"] = variants[k][1]
            e["byte_floor_us_at_8.0TBs"] = b / HBM_PEAK * 1e6
            e["fraction_of_byte_floor"] = (b / HBM_PEAK * 1e6) / e["mean_us"]
            e["fraction_of_measured_copy_rate"] = (b / HBM_MEASURED * 1e6) / e["mean_us"]
        result["variants"][k] = e
        print(f"{k:22s} {e['mean_us']:10.1f} us  (min {e['min_us']:.1f}, max {e['max_us']:.1f})",
              flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    ds.close()
    ctx.close()


if __name__ == "__main__":
    main()
