"""The closest-hit, TraceRay and camera-ray device entries (rt_closest_rays_device,
rt_trace_rays_device, rt_camera_rays_device) next to the routes that did their work before.

Per config (default C2, mirror, glass and mesh at 1920x1080), n = 2^20 device-resident rays made
by rt_camera_rays_device itself: the unjittered camera rays of the frame's 546 middle rows
(1 048 320 rays) and its first 256 once more.
  (a) closest_t_prim      rt_closest_rays_device(CH_T | CH_PRIM)
      closest_all         rt_closest_rays_device(CH_ALL)
      gbuffer_depth_prim  rt_gbuffer_device(GB_DEPTH | GB_PRIM) over the same 546 rows (0.02 %
                          fewer rays): the parent commit's code for the same work from pixels
      gbuffer_generic     the same with RT_FLAG_GENERIC_KERNEL: one thread per pixel over closest()
  (b) trace_rays_device   rt_trace_rays_device, next to the host rt_trace_rays' wall time for the
                          same rays (a host clock around calls that end in a synchronise)
  (c) camera_rays         rt_camera_rays_device of the whole frame, sample 0 and sample 1 (as if
                          aa_samples = 4), next to its store bound: 48 B per ray at 6.3 TB/s
HIP events around `--launches` back-to-back launches on the context's stream, per launch, the
routes alternating inside one process after a warm-up of each; median and min .. max of
`--repeats` repeats.

  python tools/closest_time.py [--configs c2,mirror,glass,mesh] [--out profiles/closest_time.txt]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

STORE_TBPS = 6.3   # achievable HBM store bandwidth of one MI355X, TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,mirror,glass,mesh")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from raytracingengine_amd import capi
    from raytracingengine_amd.configs import make_config

    W, H = (int(v) for v in args.size.split("x"))
    n = args.rays
    rows = min(H, n // W)
    r0 = (H - rows) // 2
    lines = ["# rt_closest_rays_device next to rt_gbuffer_device over the same camera rays,",
             "# rt_trace_rays_device next to the host rt_trace_rays, rt_camera_rays_device next to its",
             "# store bound; one MI355X; us per launch (median of the repeats, min .. max), HIP events",
             "# around back-to-back launches; see tools/closest_time.py.",
             f"# build {capi.build_info()['source_sha256'][:16]}, n = {n} rays, {args.launches} "
             f"launches per repeat, {args.repeats} repeats"]
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)

    def launch_us(fn):
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
                launch_us(fn)
        reps = {k: [] for k in routes}
        for _ in range(args.repeats):
            for k, fn in routes.items():
                reps[k].append(launch_us(fn))
        ctx.synchronize()
        return reps

    def row(k, v, extra=""):
        return (f"{k:20s} {np.median(v):10.1f} us   ({min(v):.1f} .. {max(v):.1f})"
                f"   {np.median(v) * 1e3 / n:8.3f} ns/ray{extra}")

    verdicts = []
    for name in args.configs.split(","):
        sc = make_config(name, W, H, 1)
        ds = ctx.scene(sc)
        o_rows = capi.default_opts(row_begin=r0, row_end=r0 + rows)
        o_gen = capi.default_opts(row_begin=r0, row_end=r0 + rows, flags=capi.RT_FLAG_GENERIC_KERNEL)
        with torch.cuda.stream(stream):
            d_rays = torch.empty((n, 6), dtype=torch.float64, device="cuda")
            ds.camera_rays_device(0, out=d_rays, row_begin=r0, row_end=r0 + rows)
            ctx.synchronize()
            d_rays[rows * W:] = d_rays[:n - rows * W]
            o_ch = {k: torch.empty((n, w) if w else (n,), dtype=torch.int32 if k == "prim"
                                   else torch.float64, device="cuda")
                    for k, _, _, w in capi.CH_OUTPUTS}
            o_rgb = torch.empty((n, 3), dtype=torch.float64, device="cuda")
            g_depth = torch.empty(rows * W, dtype=torch.float64, device="cuda")
            g_prim = torch.empty((rows * W, 2), dtype=torch.int32, device="cuda")
        stream.synchronize()
        gb = capi.GB_DEPTH | capi.GB_PRIM
        g_ptrs = {"depth": g_depth.data_ptr(), "prim": g_prim.data_ptr()}
        routes = {
            "closest_t_prim": lambda: ds.closest_device(d_rays, capi.CH_T | capi.CH_PRIM, out=o_ch),
            "closest_all": lambda: ds.closest_device(d_rays, capi.CH_ALL, out=o_ch),
            "gbuffer_depth_prim": lambda: ds.gbuffer_device(gb, g_ptrs, opts=o_rows),
            "gbuffer_generic": lambda: ds.gbuffer_device(gb, g_ptrs, opts=o_gen),
            "trace_rays_device": lambda: ds.trace_rays_device(d_rays, out=o_rgb),
        }
        reps = measure(routes)
        # the two routes agree on what they saw
        ds.closest_device(d_rays, capi.CH_T | capi.CH_PRIM, out=o_ch)
        ds.gbuffer_device(gb, g_ptrs, opts=o_rows)
        ctx.synchronize()
        same = bool(torch.equal(o_ch["t"][:rows * W], g_depth)
                    and torch.equal(o_ch["prim"][:rows * W], g_prim))
        hits = int((o_ch["prim"][:, 0] != 0).sum())
        # (b) the host entry's wall time for the same rays
        host = d_rays.cpu().numpy()
        ds.trace_rays(host)
        th = []
        for _ in range(3):
            t0 = time.perf_counter()
            ds.trace_rays(host)
            th.append((time.perf_counter() - t0) * 1e6)
        lines += ["", f"## {name} {W}x{H}: {n} rays, {hits} hits; closest_device == gbuffer_device "
                      f"on the shared rays: {same}"]
        for k, v in reps.items():
            lines.append(row(k, v))
        lines.append(f"{'trace_rays (host)':20s} {np.median(th):10.1f} us   ({min(th):.1f} .. {max(th):.1f})"
                     f"   wall time, upload and download included")
        print("\n".join(lines[-(len(reps) + 2):]), flush=True)
        a, b, g = reps["closest_t_prim"], reps["closest_all"], reps["gbuffer_depth_prim"]
        gg = reps["gbuffer_generic"]
        verdicts.append(f"{name}: closest T|PRIM {np.median(a):.1f} us, CH_ALL {np.median(b):.1f} us "
                        f"(x{np.median(b) / np.median(a):.2f}), gbuffer packet {np.median(g):.1f} us, "
                        f"gbuffer generic {np.median(gg):.1f} us; trace_rays_device "
                        f"{np.median(reps['trace_rays_device']):.1f} us vs host "
                        f"{np.median(th):.1f} us (x{np.median(th) / np.median(reps['trace_rays_device']):.1f})")
        ds.close()

    # (c) camera rays of the whole frame (no scene is read: c2's camera)
    sc = make_config("c2", W, H, 1)
    ds = ctx.scene(sc)
    cam4 = ds.cameras([sc.camera.position])
    cam4["aa_samples"] = 4
    with torch.cuda.stream(stream):
        d_frame = torch.empty((W * H, 6), dtype=torch.float64, device="cuda")
    stream.synchronize()
    reps = measure({"camera_rays_s0": lambda: ds.camera_rays_device(0, cam=cam4, out=d_frame),
                    "camera_rays_s1": lambda: ds.camera_rays_device(1, cam=cam4, out=d_frame)})
    bound = W * H * 48 / (STORE_TBPS * 1e12) * 1e6
    lines += ["", f"## camera rays {W}x{H}: {W * H} rays, 48 B each; store bound at {STORE_TBPS} TB/s: "
                  f"{bound:.1f} us"]
    for k, v in reps.items():
        lines.append(f"{k:20s} {np.median(v):10.1f} us   ({min(v):.1f} .. {max(v):.1f})"
                     f"   {W * H * 48 / np.median(v) / 1e6:8.2f} TB/s")
    print("\n".join(lines[-3:]), flush=True)
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
