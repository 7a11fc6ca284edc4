"""The transmittance queries (rt_transmittance_rays_device / transmittance_rays_kernel and
rt_light_transmittance_device / light_transmittance_kernel) next to the occlusion query
(rt_occluded_rays_device) on the same rays and distances.

Per config (default C2, glass and bigmesh at 1920x1080) two sets:
  camera   the unjittered camera ray of every pixel, maxDist = +inf: transmittance_rays_kernel
  light    every pixel's hit point with the normal facing the viewer: light_transmittance_kernel
           over all the scene's lights; the occlusion query is timed on the shadow rays towards
           light 0 that the kernel forms itself (origin offset by the bias, maxDist = the distance
           to the light minus the bias), and so is transmittance_rays_kernel

and per set HIP events around `--launches` back-to-back launches on the context's stream, per
launch, the routes alternating inside one process after a warm-up of each; `--repeats` repeats
give the spread.  On a scene without transparency the transmittance routes run twice, by default
(occlusion_opaque first) and with RTAMD_TX_OPAQUE=0 (the march alone), and the tool checks that
both give the same bits.  Kernel times alone come from a kernel trace, one traced process per
config and set, which only makes `--kernels-only N` launches of each route:

  python tools/transmittance_time.py [--configs c2,glass,bigmesh] [--out profiles/transmittance_time.txt]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- \
      python tools/transmittance_time.py --configs c2 --sets light --kernels-only 20
  python tools/transmittance_time.py --fold DIR_c2_light ... --out profiles/transmittance_time.txt   (appends)
"""
import argparse
import csv
import glob
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from occlusion_time import camera_rays   # tools/occlusion_time.py, next to this file

BIAS = 1e-3
KERNELS = ("light_transmittance_kernel", "transmittance_rays_kernel", "occluded_rays_kernel")


def surface_points(cam_rays, hits):
    """{hit point, normal facing the viewer} of every pixel that hit something."""
    hit = hits[:, 0] != 0
    p, n, d = hits[hit, 6:9], hits[hit, 3:6].copy(), cam_rays[hit, 3:6]
    n[(n * d).sum(-1) > 0.0] *= -1.0
    return np.ascontiguousarray(np.concatenate([p, n], -1))


def shadow_rays(sc, pts):
    """directLightning's shadow rays of the points towards light 0 (those it casts)."""
    p, n = pts[:, :3], pts[:, 3:]
    v = np.array(sc.light_array()["position"][0]) - p
    dist = np.sqrt((v * v).sum(-1))
    L = v / dist[:, None]
    cast = ((n * L).sum(-1) > 0.0) & (dist > BIAS)
    rays = np.concatenate([p + n * BIAS, L], -1)[cast]
    return np.ascontiguousarray(rays), np.ascontiguousarray(dist[cast] - BIAS)


def short_name(name):
    """'void rtamd::kernel<true>(args...)' -> 'kernel<true>'."""
    head = name.split("(")[0].split()[-1]
    return head.split("::")[-1]


def fold(dirs, out):
    """Per traced directory, the rows of its kernel_stats.csv that name one of KERNELS."""
    lines = ["", "## kernels alone (rocprofv3 --kernel-trace --stats, one traced process per set)",
             f"{'trace':22s} {'kernel':38s} {'calls':>6s} {'mean us':>10s} {'min us':>10s} {'max us':>10s}"]
    for d in dirs:
        for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
            rows = [r for r in csv.DictReader(open(path)) if any(k in r["Name"] for k in KERNELS)]
            for row in sorted(rows, key=lambda r: short_name(r["Name"])):
                lines.append(f"{os.path.basename(os.path.normpath(d)):22s} "
                             f"{short_name(row['Name']):38s} {int(row['Calls']):6d} "
                             f"{float(row['AverageNs']) / 1e3:10.1f} "
                             f"{float(row['MinNs']) / 1e3:10.1f} {float(row['MaxNs']) / 1e3:10.1f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "a") as fh:
            fh.write(text)


def set_opaque_switch(on):
    """RTAMD_TX_OPAQUE is read per launch: the process environment decides the next one."""
    if on:
        os.environ.pop("RTAMD_TX_OPAQUE", None)
    else:
        os.environ["RTAMD_TX_OPAQUE"] = "0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,glass,bigmesh")
    ap.add_argument("--sets", default="camera,light")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--launches", type=int, default=100)
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

    W, H = (int(v) for v in args.size.split("x"))
    lines = ["# Transmittance queries next to the occlusion query on the same rays, one MI355X; us per",
             "# launch over all the set's rays (mean of the repeats, min .. max), HIP events around",
             "# back-to-back launches; see tools/transmittance_time.py.",
             f"# build {capi.build_info()['source_sha256'][:16]}, {args.launches} launches per "
             f"repeat, {args.repeats} repeats"]
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    for name in args.configs.split(","):
        sc = make_config(name, W, H)
        ds = ctx.scene(sc)
        cam = camera_rays(sc)
        pts = surface_points(cam, ds.intersect_rays(cam))
        sh_rays, sh_dist = shadow_rays(sc, pts)
        opaque_scene = not any((a["material"]["transparency"] > 0.0).any() for a in
                               (sc.sphere_array(), sc.plane_array(), sc.triangle_array()))
        with torch.cuda.stream(stream):
            dev = {k: torch.from_numpy(v).cuda() for k, v in
                   dict(cam=cam, inf=np.full(len(cam), np.inf), pts=pts, sh_rays=sh_rays,
                        sh_dist=sh_dist).items()}
            T_cam = torch.empty(len(cam), dtype=torch.float64, device="cuda")
            T_sh = torch.empty(len(sh_rays), dtype=torch.float64, device="cuda")
            T_lt = torch.empty((len(pts), len(sc.lights)), dtype=torch.float64, device="cuda")
            O_cam = torch.empty(len(cam), dtype=torch.uint8, device="cuda")
            O_sh = torch.empty(len(sh_rays), dtype=torch.uint8, device="cuda")
        stream.synchronize()

        def tx_cam():
            ds.transmittance_device(dev["cam"], dev["inf"], out=T_cam)

        def occ_cam():
            ds.occluded_device(dev["cam"], dev["inf"], out=O_cam)

        def lt_all():
            ds.light_transmittance_device(dev["pts"], out=T_lt)

        def tx_sh():
            ds.transmittance_device(dev["sh_rays"], dev["sh_dist"], out=T_sh)

        def occ_sh():
            ds.occluded_device(dev["sh_rays"], dev["sh_dist"], out=O_sh)

        def with_switch(fn, on):
            def run():
                set_opaque_switch(on)
                try:
                    fn()
                finally:
                    set_opaque_switch(True)
            return run

        sets = {}
        if "camera" in args.sets.split(","):
            sets["camera"] = (len(cam), {"transmittance": tx_cam, "occluded": occ_cam}, [(tx_cam, T_cam)])
        if "light" in args.sets.split(","):
            sets["light"] = (len(pts), {"light_transmittance": lt_all, "transmittance_light0": tx_sh,
                                        "occluded_light0": occ_sh}, [(lt_all, T_lt), (tx_sh, T_sh)])
        for sname, (n, routes, checked) in sets.items():
            if opaque_scene:   # both ways, and the same bits
                for fn, buf in checked:
                    fn()
                    ctx.synchronize()
                    fast = buf.cpu().numpy().copy()
                    with_switch(fn, False)()
                    ctx.synchronize()
                    assert np.array_equal(fast.view(np.uint64), buf.cpu().numpy().view(np.uint64))
                for k in [k for k in routes if "transmittance" in k]:
                    routes[k + " RTAMD_TX_OPAQUE=0"] = with_switch(routes[k], False)
            if args.kernels_only:
                for fn in routes.values():
                    for _ in range(args.kernels_only):
                        fn()
                    ctx.synchronize()
                continue

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
            T = (T_cam if sname == "camera" else T_lt).cpu().numpy()
            lines += ["", f"## {name} {W}x{H}, {sname}: {n} {'rays' if sname == 'camera' else 'points'}"
                          f" x {1 if sname == 'camera' else len(sc.lights)} light(s), "
                          f"{100.0 * (T == 1.0).mean():.1f} % T == 1, {100.0 * (T == 0.0).mean():.1f} % T == 0"
                          + (f"; light 0 casts {len(sh_rays)} shadow rays" if sname == "light" else "")]
            for k, v in reps.items():
                lines.append(f"{k:40s} {np.mean(v):10.1f} us   ({min(v):.1f} .. {max(v):.1f})"
                             f"   {np.mean(v) * 1e3 / n:8.3f} ns/{'ray' if sname == 'camera' else 'point'}")
            print("\n".join(lines[-(len(reps) + 1):]), flush=True)
        ds.close()
    ctx.close()
    if args.out and not args.kernels_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
