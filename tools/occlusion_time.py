"""The occlusion query (rt_occluded_rays[_device], occluded_rays_kernel) against the only route
there was before it: rt_intersect_rays (intersect_rays_kernel) and `0 < t < maxDist` on the host.

Per config (default C2 and bigmesh at their BASELINE resolution, 1920x1080) two ray sets:
  camera   the unjittered camera ray of every pixel, maxDist = +inf ("does this pixel see anything")
  shadow   from every pixel's hit point (offset by the bias along the normal facing the viewer)
           towards the first light, maxDist = the distance to the light

and per set
  any_launch     rt_occluded_rays_device, HIP events around `--launches` back-to-back launches on
                 the context's stream, per launch
  any_host       rt_occluded_rays, host wall clock of the synchronous call (56 B/ray up, 1 B down)
  closest_host   rt_intersect_rays (48 B/ray up, 72 B down) + the numpy compare, host wall clock
The routes alternate inside one process after a warm-up of each; `--repeats` repeats give the
spread.  Kernel times of the two kernels alone come from a kernel trace, one traced process per
config and set, which only makes `--kernels-only N` calls of each host entry:

  python tools/occlusion_time.py [--configs c2,bigmesh] [--out profiles/anyhit_time.txt]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- \
      python tools/occlusion_time.py --configs c2 --sets shadow --kernels-only 20
  python tools/occlusion_time.py --fold DIR_c2_shadow ... --out profiles/anyhit_time.txt   (appends)
"""
import argparse
import csv
import glob
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

BIAS = 1e-3


def camera_rays(sc):
    """Camera::getRay of every pixel, unjittered, row-major."""
    W, H = sc.camera.width, sc.camera.height
    cam = np.array(sc.camera.position)
    xs = np.arange(W) - W / 2.0
    ys = H / 2.0 - np.arange(H)
    d = np.stack(np.broadcast_arrays(xs[None, :], ys[:, None], np.float64(sc.camera.focal)), -1)
    d = d + np.array([0.0, 0.0, cam[2]]) - cam
    d /= np.sqrt((d * d).sum(-1, keepdims=True))
    return np.ascontiguousarray(np.concatenate([np.broadcast_to(cam, d.shape), d], -1).reshape(-1, 6))


def shadow_rays(sc, cam_rays, hits):
    """directLightning's shadow ray of every pixel that hit something, towards light 0."""
    hit = hits[:, 0] != 0
    p, n, d = hits[hit, 6:9], hits[hit, 3:6].copy(), cam_rays[hit, 3:6]
    n[(n * d).sum(-1) > 0.0] *= -1.0
    o = p + n * BIAS
    v = np.array(sc.light_array()["position"][0]) - o
    dist = np.sqrt((v * v).sum(-1))
    return np.ascontiguousarray(np.concatenate([o, v / dist[:, None]], -1)), dist


def ray_sets(ds, sc, which):
    cam = camera_rays(sc)
    out = {}
    if "camera" in which:
        out["camera"] = (cam, np.full(len(cam), np.inf))
    if "shadow" in which:
        out["shadow"] = shadow_rays(sc, cam, ds.intersect_rays(cam))
    return out


def closest_route(ds, rays, dist):
    t = ds.intersect_rays(rays)
    return (t[:, 0] != 0) & (t[:, 2] > 0.0) & (t[:, 2] < dist)


def fold(dirs, out):
    """Per traced directory, the two kernels' rows of its kernel_stats.csv."""
    lines = ["", "## kernels alone (rocprofv3 --kernel-trace --stats, one traced process per set)",
             f"{'trace':28s} {'kernel':24s} {'calls':>6s} {'mean us':>10s} {'min us':>10s} {'max us':>10s}"]
    for d in dirs:
        for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
            for row in csv.DictReader(open(path)):
                for k in ("occluded_rays_kernel", "intersect_rays_kernel"):
                    if k in row["Name"]:
                        lines.append(f"{os.path.basename(os.path.normpath(d)):28s} {k:24s} "
                                     f"{int(row['Calls']):6d} {float(row['AverageNs']) / 1e3:10.1f} "
                                     f"{float(row['MinNs']) / 1e3:10.1f} {float(row['MaxNs']) / 1e3:10.1f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "a") as fh:
            fh.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,bigmesh")
    ap.add_argument("--sets", default="camera,shadow")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernels-only", type=int, default=0)
    ap.add_argument("--fold", nargs="*", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.fold is not None:
        return fold(args.fold, args.out)

    import torch

    from raytracingengine_amd import capi
    from raytracingengine_amd.configs import make_config

    lines = ["# Occlusion query against closest-hit-then-compare, one MI355X; us per call over all",
             "# the set's rays (mean of the repeats, min .. max); see tools/occlusion_time.py.",
             f"# build {capi.build_info()['source_sha256'][:16]}, {args.launches} launches per "
             f"repeat, {args.host_calls} host calls per repeat, {args.repeats} repeats"]
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    for name in args.configs.split(","):
        sc = make_config(name)
        ds = ctx.scene(sc)
        sets = ray_sets(ds, sc, args.sets.split(","))
        for sname, (rays, dist) in sets.items():
            n = len(rays)
            if args.kernels_only:
                for _ in range(args.kernels_only):
                    ds.occluded(rays, dist)
                    ds.intersect_rays(rays)
                continue
            any_hit = ds.occluded(rays, dist)
            route = closest_route(ds, rays, dist)
            with torch.cuda.stream(stream):
                d_rays = torch.from_numpy(rays).cuda()
                d_dist = torch.from_numpy(dist).cuda()
                d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
            stream.synchronize()
            ds.occluded_device(d_rays, d_dist, out=d_out)
            ctx.synchronize()
            assert np.array_equal(d_out.cpu().numpy(), any_hit.view(np.uint8))

            def launch_us():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(args.launches):
                    ds.occluded_device(d_rays, d_dist, out=d_out)
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1) * 1e3 / args.launches

            def wall_us(fn):
                t0 = time.perf_counter()
                for _ in range(args.host_calls):
                    fn()
                return (time.perf_counter() - t0) * 1e6 / args.host_calls

            routes = {"any_launch": launch_us,
                      "any_host": lambda: wall_us(lambda: ds.occluded(rays, dist)),
                      "closest_host": lambda: wall_us(lambda: closest_route(ds, rays, dist))}
            t_end = time.perf_counter() + 0.3   # warm-up past the clock ramp
            while time.perf_counter() < t_end:
                launch_us()
            for k in ("any_host", "closest_host"):
                routes[k]()
            reps = {k: [] for k in routes}
            for _ in range(args.repeats):
                for k, fn in routes.items():
                    reps[k].append(fn())
            lines += ["", f"## {name} {sc.camera.width}x{sc.camera.height}, {sname}: {n} rays, "
                          f"{100.0 * any_hit.mean():.1f} % occluded, "
                          f"{int((any_hit != route).sum())} rays answered differently by the "
                          "closest-hit route (a plane at t == 0)"]
            for k, v in reps.items():
                lines.append(f"{k:14s} {np.mean(v):12.1f} us   ({min(v):.1f} .. {max(v):.1f})"
                             f"   {np.mean(v) * 1e3 / n:8.3f} ns/ray")
            print("\n".join(lines[-4:]), flush=True)
        ds.close()
    ctx.close()
    if args.out and not args.kernels_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
