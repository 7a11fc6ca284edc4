"""The keyed queries (the keyed_ kernels: the scatter, direct-light and shadow queries with the
area light served) on C5 next to the kernel that already shades the same hits inside a frame.

Per size (default 1920x1080 and C5's own 3840x2160, one sample per pixel):
  keyed_scatter       rt_scatter_rays_keyed_device, RT_SC_VALUE, on camera_rays_device(0) under the
                      frame's keys (pixel = y*W + x, sample 0, depth 0): C5 is opaque without
                      mirrors, so this is the whole TraceRay of every pixel
  keyed_direct_rays   rt_direct_light_rays_keyed_device, RT_DL_RADIANCE, on the same rays and keys
  accumulate          rt_accumulate_samples_device(0, 1): the same TraceRay through the generic
                      trace kernel, which forms its camera rays itself
  keyed_shadow_points rt_light_transmittance_keyed_device on the hit points of those rays
                      {p, normal facing the viewer}: 16 transmittances per point
HIP events around `--launches` back-to-back launches on the context's stream, per launch, the
routes alternating inside one process after a warm-up of each; `--repeats` repeats give the
spread.  The tool checks that keyed_scatter and accumulate give the same bits, and reports the
ratio of the two with the run-to-run spread next to it.

  python tools/area_queries_time.py [--sizes 1920x1080,3840x2160] [--out profiles/area_queries_time.txt]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from raytracingengine_amd import capi
    from raytracingengine_amd.configs import make_config

    lines = ["# The keyed queries on C5 (64 spheres, one area light of 16 samples) next to",
             "# rt_accumulate_samples_device(0, 1), the generic trace kernel on the same pixels, one",
             "# MI355X; us per launch (mean of the repeats, min .. max), HIP events around back-to-back",
             "# launches, the routes interleaved; see tools/area_queries_time.py.",
             f"# build {capi.build_info()['source_sha256'][:16]}, {args.launches} launches per "
             f"repeat, {args.repeats} repeats"]
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    verdicts = []
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        sc = make_config("c5", W, H, 1)
        ds = ctx.scene(sc)
        n = W * H
        with torch.cuda.stream(stream):
            d_cam = ds.camera_rays_device(0)
            pix = torch.arange(n, dtype=torch.int64, device="cuda")
            cl = ds.closest_device(d_cam, capi.CH_PRIM | capi.CH_NORMAL | capi.CH_POINT)
            stream.synchronize()
            hit = cl["prim"][:, 0] != 0
            nrm, d = cl["normal"][hit], d_cam[hit, 3:]
            front = (nrm * d).sum(dim=1) < 0.0   # the sign only: d is a positive multiple of incoming
            d_pn = torch.cat([cl["point"][hit], torch.where(front[:, None], nrm, -nrm)], 1).contiguous()
            hit_pix = pix[hit].contiguous()
            m = len(d_pn)
            o_sc = {"value": torch.empty((n, 3), dtype=torch.float64, device="cuda")}
            o_dl = {"radiance": torch.empty((n, 3), dtype=torch.float64, device="cuda")}
            acc = torch.empty((n, 3), dtype=torch.float64, device="cuda")
            T = torch.empty((m, sc.area_light.samples), dtype=torch.float64, device="cuda")
        stream.synchronize()
        keys, pkeys = capi.AreaKeys(pix), capi.AreaKeys(hit_pix)
        routes = {
            "keyed_scatter": lambda: ds.scatter_device(d_cam, capi.SC_VALUE, out=o_sc, area_keys=keys),
            "keyed_direct_rays": lambda: ds.direct_light_rays_device(d_cam, capi.DL_RADIANCE, out=o_dl,
                                                                     area_keys=keys),
            "accumulate": lambda: ds.accumulate_device(0, 1, sum=acc),
            "keyed_shadow_points": lambda: ds.light_transmittance_device(d_pn, out=T, area_keys=pkeys),
        }
        for fn in routes.values():
            fn()
        ctx.synchronize()
        a, b = o_sc["value"].cpu().numpy(), acc.cpu().numpy()
        same = np.array_equal(a.view(np.uint64), b.view(np.uint64))
        soft = T.mean(dim=1)
        penumbra = int(((soft > 0) & (soft < 1)).sum())

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
        lines += ["", f"## c5 {W}x{H}: {n} camera rays, {m} hit points ({penumbra} in the penumbra); "
                      f"keyed_scatter == accumulate(0, 1) bit for bit: {same}"]
        for k, v in reps.items():
            cnt = m if k == "keyed_shadow_points" else n
            lines.append(f"{k:20s} {np.mean(v):10.1f} us   ({min(v):.1f} .. {max(v):.1f})"
                         f"   {np.mean(v) * 1e3 / cnt:8.3f} ns/{'point' if cnt == m else 'ray'}")
        ks, ac = reps["keyed_scatter"], reps["accumulate"]
        ratio = np.mean(ks) / np.mean(ac)
        spread = max(max(ks) - min(ks), max(ac) - min(ac))
        diff = np.mean(ks) - np.mean(ac)
        lines.append(f"keyed_scatter / accumulate = {ratio:.3f}")
        verdicts.append(f"c5 {W}x{H}: keyed_scatter {np.mean(ks):.1f} us vs accumulate {np.mean(ac):.1f} us, "
                        f"ratio {ratio:.3f}, run-to-run spread {spread:.1f} us: "
                        + ("within the spread" if abs(diff) <= spread
                           else ("slower beyond the spread" if diff > 0 else "faster beyond the spread")))
        print("\n".join(lines[-(len(reps) + 2):]), flush=True)
        ds.close()
    ctx.close()
    lines += ["", "## keyed scatter against the generic trace kernel on the same pixels"] + verdicts
    print("\n".join(lines[-(len(verdicts) + 1):]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
