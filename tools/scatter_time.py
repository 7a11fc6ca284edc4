"""The scatter query (rt_scatter_rays_device / scatter_rays_kernel) next to
rt_direct_light_rays_device on the same rays — the same closest hit and light loop, 24 B out —
and the level-by-level composition next to rt_trace_rays.

Per config (default C2, mirror and glass at 1920x1080), n = 2^20 device-resident rays: the
unjittered camera rays of the frame's middle rows (cycled if the frame has fewer than n):
  (a) direct_light_rays   rt_direct_light_rays_device(DL_RADIANCE): the yardstick
  (b) scatter_value       rt_scatter_rays_device(SC_VALUE)
  (c) scatter_all         rt_scatter_rays_device(SC_ALL)
  (d) scatter_children    rt_scatter_rays_device(SC_ALL & ~SC_VALUE): no light loop
HIP events around `--launches` back-to-back launches on the context's stream, per launch, the
routes alternating inside one process after a warm-up of each; median and min .. max of
`--repeats` repeats.
  (e) capi.compose_trace to max_recursion `--depth` next to rt_trace_rays at the same depth, both
      from host rays to host colours (a host clock around calls that end in a synchronise), on
      the first `--compose-rays` of the rays.

  python tools/scatter_time.py [--configs c2,mirror,glass] [--out profiles/scatter_time.txt]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from occlusion_time import camera_rays   # tools/occlusion_time.py, next to this file


def pick_rays(cam, n):
    """n rays of the frame: its middle (whole rows are not needed), cycled if it has fewer."""
    if len(cam) >= n:
        at = (len(cam) - n) // 2
        return np.ascontiguousarray(cam[at:at + n])
    return np.ascontiguousarray(np.resize(cam, (n, 6)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,mirror,glass")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--compose-rays", type=int, default=1 << 18)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from raytracingengine_amd import capi
    from raytracingengine_amd.configs import make_config

    W, H = (int(v) for v in args.size.split("x"))
    n = args.rays
    lines = ["# The scatter query next to rt_direct_light_rays_device on the same rays, one MI355X; us per",
             "# launch (median of the repeats, min .. max), HIP events around back-to-back launches;",
             "# compose_trace and rt_trace_rays host to host, ms per call; see tools/scatter_time.py.",
             f"# build {capi.build_info()['source_sha256'][:16]}, n = {n} rays, {args.launches} "
             f"launches per repeat, {args.repeats} repeats"]
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    verdicts = []
    for name in args.configs.split(","):
        sc = make_config(name, W, H, 1)
        ds = ctx.scene(sc)
        rays = pick_rays(camera_rays(sc), n)
        with torch.cuda.stream(stream):
            d_rays = torch.from_numpy(rays).cuda()
            o_dl = {"radiance": torch.empty((n, 3), dtype=torch.float64, device="cuda")}
            o_sc = {k: torch.empty((n, w) if w else (n,), dtype=torch.uint8 if k == "flags"
                                   else torch.float64, device="cuda")
                    for k, _, _, w in capi.SC_OUTPUTS}
        stream.synchronize()
        children = capi.SC_ALL & ~capi.SC_VALUE
        routes = {
            "direct_light_rays": lambda: ds.direct_light_rays_device(d_rays, out=o_dl),
            "scatter_value": lambda: ds.scatter_device(d_rays, capi.SC_VALUE, out=o_sc),
            "scatter_all": lambda: ds.scatter_device(d_rays, capi.SC_ALL, out=o_sc),
            "scatter_children": lambda: ds.scatter_device(d_rays, children, out=o_sc),
        }
        for fn in routes.values():
            fn()
        ctx.synchronize()
        flags = o_sc["flags"].cpu().numpy()

        def launch_us(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.launches):
                fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / args.launches

        t_end = time.perf_counter() + 0.3   # warm-up past the clock ramp
        while time.perf_counter() < t_end:
            for fn in routes.values():
                launch_us(fn)
        reps = {k: [] for k in routes}
        for _ in range(args.repeats):
            for k, fn in routes.items():
                reps[k].append(launch_us(fn))
        ctx.synchronize()
        lines += ["", f"## {name} {W}x{H}: {n} rays, {int((flags & 1 != 0).sum())} hits, "
                      f"{int((flags & 2 != 0).sum())} refraction and {int((flags & 4 != 0).sum())} "
                      f"reflection children; {len(sc.lights)} light(s)"]
        for k, v in reps.items():
            lines.append(f"{k:18s} {np.median(v):10.1f} us   ({min(v):.1f} .. {max(v):.1f})"
                         f"   {np.median(v) * 1e3 / n:8.3f} ns/ray")
        a, b = reps["direct_light_rays"], reps["scatter_value"]
        c, d = reps["scatter_all"], reps["scatter_children"]
        spread = max(max(a) - min(a), max(b) - min(b))
        ok = abs(np.median(b) - np.median(a)) <= spread
        verdicts.append(f"{name}: scatter_value {np.median(b):.1f} us vs direct_light_rays "
                        f"{np.median(a):.1f} us, run-to-run spread {spread:.1f} us: "
                        + ("within the spread" if ok else "NOT within the spread")
                        + f"; all / value = {np.median(c) / np.median(b):.3f}, "
                          f"children / value = {np.median(d) / np.median(b):.3f}")
        # (e) the composition, host to host
        m = min(n, args.compose_rays)
        host = rays[:m]
        ds.trace_rays(host, max_recursion=args.depth)
        capi.compose_trace(ds, host, args.depth)
        te, tc = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            traced = ds.trace_rays(host, max_recursion=args.depth)
            t1 = time.perf_counter()
            composed = capi.compose_trace(ds, host, args.depth)
            t2 = time.perf_counter()
            te.append((t1 - t0) * 1e3)
            tc.append((t2 - t1) * 1e3)
        err = np.abs(composed - traced) / np.maximum(1.0, np.abs(traced))
        lines.append(f"compose_trace      {np.median(tc):10.1f} ms   ({min(tc):.1f} .. {max(tc):.1f})   "
                     f"rt_trace_rays {np.median(te):.1f} ms ({min(te):.1f} .. {max(te):.1f}); "
                     f"{m} rays, depth {args.depth}, max scaled difference {err.max():.2e}")
        print("\n".join(lines[-(len(reps) + 2):]), flush=True)
        ds.close()
    ctx.close()
    lines += ["", "## scatter_value against direct_light_rays_kernel on the same rays"] + verdicts
    print("\n".join(lines[-(len(verdicts) + 1):]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
