"""Adaptive progressive frames (rt_accumulate_adaptive_device) next to the parent's
accumulate_device(0, N) and rt_render_device, measured in the same run.

Per config (default C1's own 1000x1000 at aa_samples = 32, the reference main()'s, and c5 at its
BASELINE 3840x2160 with aa_samples = 8), for a handful of tolerances and for the never-converging
rule (min_samples = N: the price of the moments and the rule), each with the list kernel on and
off (RTAMD_ADAPT_LIST, read per call):
  time       one fresh accumulate_adaptive_device(N) per frame, us, next to
             acc     accumulate_device(0, N), the sum every pixel takes all N samples of
             render  rt_render_device, for information (its packet / box kernels are not the
                     generic TraceRay the sample ranges run)
  traced     count.sum() / (N * pixels): the share of samples traced
  listed     the share of pixels the tile kernel handed to the list kernel
  error      mean and maximum |adaptive - full| over the float64 frame (resolve_counts_device
             against resolve_device(accumulate_device(0, N), N)) and the count of differing ACES
             bytes
HIP events around `--launches` back-to-back frames on the context's stream, per frame, the routes
alternating inside one process after a warm-up of each; median and min .. max of `--repeats`
repeats.  A route beats another only beyond the min .. max spread of both.

  python tools/adaptive_time.py [--configs c1:1000x1000:32,c5:3840x2160:8]
                                [--tolerances 0.2,0.1,0.05,0.02,0.01] [--min-samples 4]
                                [--out profiles/adaptive_time.txt]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

ACES = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c1:1000x1000:32,c5:3840x2160:8")
    ap.add_argument("--tolerances", default="0.2,0.1,0.05,0.02,0.01")
    ap.add_argument("--min-samples", type=int, default=4)
    ap.add_argument("--lum-floor", type=float, default=0.01)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from raytracingengine_amd import capi
    from raytracingengine_amd.configs import make_config

    lines = ["# accumulate_adaptive_device (fresh, to N samples) next to accumulate_device(0, N) and",
             "# rt_render_device; one MI355X; us per frame (median of the repeats, min .. max), HIP events",
             "# around back-to-back frames on one stream; see tools/adaptive_time.py.",
             f"# build {capi.build_info()['source_sha256'][:16]}, {args.launches} frames per repeat, "
             f"{args.repeats} repeats, min_samples {args.min_samples}, lum_floor {args.lum_floor}"]
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

    tolerances = [float(t) for t in args.tolerances.split(",")]
    for spec in args.configs.split(","):
        name, size, aa = spec.split(":")
        W, H = (int(v) for v in size.split("x"))
        N = int(aa)
        ds = ctx.scene(make_config(name, W, H, N))
        px = W * H
        o = capi.default_opts()
        with torch.cuda.stream(stream):
            d_sum = torch.empty((px, 3), dtype=torch.float64, device="cuda")
            d_frame = torch.empty((px, 3), dtype=torch.float64, device="cuda")
            state = capi.AdaptiveState(torch.empty((px, 3), dtype=torch.float64, device="cuda"),
                                       torch.empty((px, 2), dtype=torch.float64, device="cuda"),
                                       torch.empty((px,), dtype=torch.int32, device="cuda"))
        stream.synchronize()

        def adaptive(tol, min_samples, listing):
            def run():
                os.environ["RTAMD_ADAPT_LIST"] = "1" if listing else "0"
                ds.accumulate_adaptive_device(N, tol, min_samples, args.lum_floor, state=state,
                                              fresh=True)
            return run

        rules = [(f"tol {t:g}", t, args.min_samples) for t in tolerances]
        rules.append(("never", 0.0, max(N, 2)))
        routes = {"acc": lambda: ds.accumulate_device(0, N, sum=d_sum),
                  "render": lambda: ds.render_device(d_frame.data_ptr(), None, None, o)}
        for label, tol, ms in rules:
            for listing in (True, False):
                routes[f"{label} list {'on' if listing else 'off'}"] = adaptive(tol, ms, listing)

        # the frames' content, once per rule and switch, before timing
        routes["acc"]()
        full = ds.resolve_device(d_sum, N, tonemap=ACES)
        ctx.synchronize()
        full64, full_ldr = full["hdr64"].clone(), full["ldr"].clone()
        stats = {}
        for label, tol, ms in rules:
            kept = None
            for listing in (True, False):
                key = f"{label} list {'on' if listing else 'off'}"
                routes[key]()
                listed = ctx.debug_adaptive_listed()
                got = ds.resolve_counts_device(state.sum, state.count, tonemap=ACES)
                ctx.synchronize()
                diff = (got["hdr64"] - full64).abs()
                stats[key] = dict(traced=float(state.count.sum().item()) / (N * px),
                                  listed=listed / px, mean=float(diff.mean().item()),
                                  max=float(diff.max().item()),
                                  bytes=int((got["ldr"] != full_ldr).sum().item()))
                now = tuple(t.clone() for t in state)
                if kept is not None:
                    stats[key]["same"] = all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                                             for a, b in zip(kept, now))
                kept = now
        reps = measure(routes)
        os.environ.pop("RTAMD_ADAPT_LIST", None)
        med = {k: float(np.median(v)) for k, v in reps.items()}
        block = ["", f"## {name} {W}x{H}, aa_samples = {N} ({px} pixels)"]
        for k in ("acc", "render"):
            v = reps[k]
            block.append(f"{k:22s} {med[k]:11.1f} us   ({min(v):.1f} .. {max(v):.1f})")
        for k, s in stats.items():
            v = reps[k]
            same = "" if "same" not in s else f"  bits == list on: {s['same']}"
            block.append(f"{k:22s} {med[k]:11.1f} us   ({min(v):.1f} .. {max(v):.1f})  "
                         f"/acc {med[k] / med['acc']:.3f}  traced {s['traced']:.4f}  "
                         f"listed {s['listed']:.4f}  |d| mean {s['mean']:.3e} max {s['max']:.3e}  "
                         f"ACES bytes differing {s['bytes']}{same}")
        lines += block
        print("\n".join(block), flush=True)
        ds.close()

    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
