"""The direct-lighting queries (rt_direct_light_rays_device / direct_light_rays_kernel and
rt_direct_light_device / direct_light_points_kernel) next to the two routes a caller had before
them: rt_light_transmittance_device on the same points (the same marches, no colour) and the
whole-frame render of the same camera.

Per config (default C2, C4, glass and bigmesh at 1920x1080, one sample per pixel):
  rays            rt_direct_light_rays_device on the unjittered camera ray of every pixel
  points          rt_direct_light_device on those rays' hit points {p, normal facing the viewer,
                  view}, one material per point (the hit primitive's)
  points_shared   the same points with one material for all of them (in the kernel arguments)
  light_transmittance   rt_light_transmittance_device on the same points {p, normal}
  render          rt_render_device of the same camera into a float64 frame
HIP events around `--launches` back-to-back launches on the context's stream, per launch, the
routes alternating inside one process after a warm-up of each; `--repeats` repeats give the
spread.  The tool also checks that the rays entry and the points entry give the same bits.

  python tools/direct_light_time.py [--configs c2,c4,glass,bigmesh] [--out profiles/direct_light_time.txt]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from occlusion_time import camera_rays   # tools/occlusion_time.py, next to this file


def shading_points(sc, cam_rays, hits):
    """(index of the pixels that hit, points [m, 9] {p, normal facing the viewer, view},
    materials [m, 7] of the hit primitives)."""
    idx = np.flatnonzero(hits[:, 0] != 0)
    h, d = hits[idx], cam_rays[idx, 3:6]
    # incoming = d.normalize() and the flip of Scene.h:144-146, in the reference's operation order
    ln = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    inc = d / ln[:, None]
    n = h[:, 3:6]
    front = n[:, 0] * inc[:, 0] + n[:, 1] * inc[:, 1] + n[:, 2] * inc[:, 2] < 0.0
    n = np.where(front[:, None], n, -n)
    pts = np.ascontiguousarray(np.concatenate([h[:, 6:9], n, -inc], -1))
    mats = np.zeros((len(idx), 7), np.float64)
    for kind, arr in ((1, sc.sphere_array()), (2, sc.plane_array()), (3, sc.triangle_array())):
        sel = h[:, 0] == kind
        if sel.any():
            m = arr["material"][h[sel, 1].astype(np.int64)]
            mats[sel] = np.concatenate([m["color"], m["shininess"][:, None], m["specular"][:, None],
                                        m["transparency"][:, None], m["refractive_index"][:, None]], 1)
    return idx, pts, mats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c4,glass,bigmesh")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from raytracingengine_amd import capi
    from raytracingengine_amd.configs import make_config

    W, H = (int(v) for v in args.size.split("x"))
    lines = ["# Direct-lighting queries next to rt_light_transmittance_device on the same points and the",
             "# whole-frame render of the same camera, one MI355X; us per launch (mean of the repeats,",
             "# min .. max), HIP events around back-to-back launches; see tools/direct_light_time.py.",
             f"# build {capi.build_info()['source_sha256'][:16]}, {args.launches} launches per "
             f"repeat, {args.repeats} repeats"]
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    verdicts = []
    for name in args.configs.split(","):
        sc = make_config(name, W, H, 1)
        ds = ctx.scene(sc)
        cam = camera_rays(sc)
        idx, pts, mats = shading_points(sc, cam, ds.intersect_rays(cam))
        n_spec = int(((mats[:, 4] > 0.0) & (mats[:, 5] <= 0.0)).sum())
        with torch.cuda.stream(stream):
            d_cam = torch.from_numpy(cam).cuda()
            d_pts = torch.from_numpy(pts).cuda()
            d_pn = torch.from_numpy(np.ascontiguousarray(pts[:, :6])).cuda()
            d_mat = torch.from_numpy(mats).cuda()
            o_rays = {"radiance": torch.empty((len(cam), 3), dtype=torch.float64, device="cuda")}
            o_pts = {"radiance": torch.empty((len(pts), 3), dtype=torch.float64, device="cuda")}
            o_sh = {"radiance": torch.empty((len(pts), 3), dtype=torch.float64, device="cuda")}
            T = torch.empty((len(pts), len(sc.lights)), dtype=torch.float64, device="cuda")
            frame = torch.empty((H, W, 3), dtype=torch.float64, device="cuda")
        stream.synchronize()
        shared = tuple(mats[0])
        opts = capi.default_opts(tonemap=capi.TONEMAP_NONE)

        routes = {
            "rays": lambda: ds.direct_light_rays_device(d_cam, out=o_rays),
            "points": lambda: ds.direct_light_device(d_pts, d_mat, out=o_pts),
            "points_shared": lambda: ds.direct_light_device(d_pts, shared, out=o_sh),
            "light_transmittance": lambda: ds.light_transmittance_device(d_pn, out=T),
            "render": lambda: ds.render_device(frame.data_ptr(), None, None, opts),
        }
        per = {"rays": len(cam), "render": len(cam)}
        for fn in routes.values():
            fn()
        ctx.synchronize()
        a, b = o_rays["radiance"].cpu().numpy()[idx], o_pts["radiance"].cpu().numpy()
        same = np.array_equal(a.view(np.uint64), b.view(np.uint64))

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
        lines += ["", f"## {name} {W}x{H}: {len(cam)} camera rays, {len(pts)} hit points x "
                      f"{len(sc.lights)} light(s); {n_spec} points with an opaque specular material "
                      f"(pow can be reached); rays entry == points entry bit for bit: {same}"]
        for k, v in reps.items():
            n = per.get(k, len(pts))
            lines.append(f"{k:22s} {np.mean(v):10.1f} us   ({min(v):.1f} .. {max(v):.1f})"
                         f"   {np.mean(v) * 1e3 / n:8.3f} ns/{'ray' if k in per else 'point'}")
        lt, p = reps["light_transmittance"], reps["points"]
        ratio = np.mean(p) / np.mean(lt)
        lines.append(f"points / light_transmittance = {ratio:.3f}; rays / render = "
                     f"{np.mean(reps['rays']) / np.mean(reps['render']):.3f}")
        if n_spec == 0:
            spread = max(max(lt) - min(lt), max(p) - min(p))
            ok = abs(np.mean(p) - np.mean(lt)) <= spread
            verdicts.append(f"{name}: points {np.mean(p):.1f} us vs light_transmittance {np.mean(lt):.1f} us,"
                            f" run-to-run spread {spread:.1f} us: "
                            + ("within the spread" if ok else "NOT within the spread"))
        else:
            verdicts.append(f"{name}: pow is reached, ratio only: {ratio:.3f}")
        print("\n".join(lines[-(len(reps) + 2):]), flush=True)
        ds.close()
    ctx.close()
    lines += ["", "## points entry against light_transmittance_kernel on the same points"] + verdicts
    print("\n".join(lines[-(len(verdicts) + 1):]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
