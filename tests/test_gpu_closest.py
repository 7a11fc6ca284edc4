"""rt_camera_rays[_device] (rt_camera_rays.hip), rt_closest_rays[_device] (rt_closest.hip) and
rt_trace_rays_device: the renderer's own primary rays, the closest hit with selectable outputs
and TraceRay on device pointers, on the 648-ray sets of tests/raysets.py and the 24x16 frame.

The comparators are the parent's entries, already pinned to the oracle: rt_intersect_rays for
the closest hit, rt_trace_rays for the trace, rt_render and rt_gbuffer for the frame, and the
oracle's Camera::getRay for the rays.  Comparisons are as bits unless said otherwise."""
import os
import subprocess

import numpy as np
import pytest
import torch

import direct_light_sets as dl
import raysets
import scatter_sets as ss
from raytracingengine_amd import capi
from raytracingengine_amd.configs import make_config

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "bin", "closest_scenefile")
SCENES = raysets.GOLDEN_SCENES + ["sph300", "glass_tri_area"]
SIZES = (0, 1, 63, 64, 65, 255, 256, 257)
GUARD = 64
FILL = -7.25          # the guard value of the float64 outputs: no distance, normal, point, material
FILL_I32 = -77        # and of prim: no type, no index
WIDTH = {"t": 1, "prim": 2, "normal": 3, "point": 3, "material": 7}
BITS = {"t": capi.CH_T, "prim": capi.CH_PRIM, "normal": capi.CH_NORMAL, "point": capi.CH_POINT,
        "material": capi.CH_MATERIAL}
SEED = 0x5EED         # rt_render_opts_default's
W, H = raysets.SIZE
CYCLIC = dict(row_block=2, row_cycle=3, row_begin=2)
# The composed frame on the chain scenes: the largest difference, scaled by max(1, |v|), between
# the two parent-code paths rt_render and rt_trace_rays over raysets.camera_rays at aa_samples = 1
# (measured on one MI355X; the chain render kernels accumulate front to back).
# Where it is 0 the composed frame is held to bits, else to four times it: four samples summed.
PARENT_RENDER_VS_TRACE = {"mirror": 0.0, "c1": 0.0}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_same(got, want, what):
    """Equal dtype, shape and bytes (float64 as bits: -0.0 is not +0.0, a NaN would show)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    a = bits(got) if got.dtype == np.float64 else got
    b = bits(want) if want.dtype == np.float64 else want
    bad = np.flatnonzero((a != b).reshape(len(got), -1).any(axis=1)) if got.size else []
    assert not len(bad), (what, len(bad), bad[:8], got[bad[:4]], want[bad[:4]])


def assert_outputs_same(a, b, what):
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for k in a:
        assert_same(a[k], b[k], (what, k))


def from_intersect(inter, sc):
    """The five outputs as rt_intersect_rays' [n, 9] rows and the scene's material table give
    them, with the miss rule of the new entries: t +inf, prim {0, -1}, +0.0 elsewhere."""
    hit = inter[:, 0] != 0
    tables = dl.scene_materials(sc)
    mat = np.zeros((len(inter), 7), np.float64)
    for k in (1, 2, 3):
        sel = inter[:, 0] == k
        if sel.any():
            mat[sel] = tables[k - 1][inter[sel, 1].astype(np.int64)]
    return {"t": np.where(hit, inter[:, 2], np.inf), "prim": inter[:, :2].astype(np.int32),
            "normal": np.ascontiguousarray(inter[:, 3:6]), "point": np.ascontiguousarray(inter[:, 6:9]),
            "material": mat}


@pytest.fixture(scope="module")
def world(ctx, oracle):
    """Per scene, made once and left unchanged: the scene, its ray set, the scene on the device
    (with its area light, where it has one), the parent's rt_intersect_rays answer and the
    device's CH_ALL answer."""
    cache = {}

    def get(name):
        if name not in cache:
            sc = raysets.scene(name)
            rays, _ = raysets.rayset(sc)
            ds = ctx.scene(sc)
            inter = ds.intersect_rays(rays)
            cache[name] = dict(sc=sc, rays=rays, ds=ds, inter=inter, got=ds.closest(rays))
        return cache[name]
    yield get
    for w in cache.values():
        w["ds"].close()


def frame_scene(name, aa=4):
    return make_config(name, W, H, aa=aa)


# ------------------------------------------------------------------ closest hit, values
@pytest.mark.parametrize("name", SCENES)
def test_closest_values(world, oracle, name):
    w = world(name)
    sc, rays, inter, got = w["sc"], w["rays"], w["inter"], w["got"]
    n = len(rays)
    assert got["t"].shape == (n,) and got["prim"].shape == (n, 2) and got["prim"].dtype == np.int32
    assert got["material"].shape == (n, 7)
    assert_outputs_same(got, from_intersect(inter, sc), name)
    hit = inter[:, 0] != 0
    # the miss rule: t = +inf, prim = {0, -1}, +0.0 elsewhere
    assert np.isposinf(got["t"][~hit]).all() and np.isfinite(got["t"][hit]).all()
    assert (got["prim"][~hit] == [0, -1]).all()
    for k in ("normal", "point", "material"):
        assert not bits(got[k][~hit]).any(), (name, k)
    # the oracle says the set is not vacuous
    ref = oracle.closest_rays(sc, rays)
    assert (ref[:, 0] != 0).sum() >= 100 and (ref[:, 0] == 0).sum() >= 1
    assert np.array_equal(ref[:, 0] != 0, hit)
    # the copies of ray 0 give ray 0's rows
    for i in raysets.repeat_indices(n):
        for k in WIDTH:
            assert got[k][i].tobytes() == got[k][0].tobytes(), (name, k, i)


@pytest.mark.parametrize("name", ("c2", "glass", "mesh", "glass_tri_area"))
def test_closest_nonfinite_rays(world, name):
    """Zero, NaN, infinite, huge and denormal o and d: the call returns, prim is
    rt_intersect_rays', and every finite value of rt_intersect_rays' hit rows is there bit for
    bit (NaN where it has NaN)."""
    w = world(name)
    rays = raysets.nonfinite_rays(w["sc"])
    inter = w["ds"].intersect_rays(rays)
    got = w["ds"].closest(rays)
    assert_same(got["prim"], inter[:, :2].astype(np.int32), (name, "prim"))
    hit = inter[:, 0] != 0
    assert np.isposinf(got["t"][~hit]).all()
    cols = {"t": inter[:, 2:3], "normal": inter[:, 3:6], "point": inter[:, 6:9]}
    for k, ref in cols.items():
        g = got[k].reshape(len(rays), -1)[hit]
        r = ref[hit]
        fin = np.isfinite(r)
        assert np.array_equal(bits(g)[fin], bits(r)[fin]), (name, k)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (name, k)
    finite = np.flatnonzero((rays == rays[2]).all(axis=1))   # the ordinary ray, three times
    assert len(finite) == 3
    full = from_intersect(inter, w["sc"])
    for k in WIDTH:
        assert_same(got[k][finite], full[k][finite], (name, k, "finite rows"))


# ------------------------------------------------------------------ output subsets and options
@pytest.mark.parametrize("name", ("c2", "glass", "mesh"))
def test_closest_output_subsets_equal_the_full_call(world, name):
    """Each single output bit and T | PRIM: the slice of CH_ALL bit for bit (the kernel's two
    instances agree)."""
    w = world(name)
    for outputs in list(BITS.values()) + [capi.CH_T | capi.CH_PRIM]:
        got = w["ds"].closest(w["rays"], outputs=outputs)
        want = {k: w["got"][k] for k, b in BITS.items() if outputs & b}
        assert_outputs_same(got, want, (name, hex(outputs)))
    for bad in (0, 0x20, 0x3f):
        with pytest.raises(ValueError):
            w["ds"].closest(w["rays"], outputs=bad)


def test_closest_no_bvh_equals_bvh(world):
    w = world("mesh")
    assert_outputs_same(w["ds"].closest(w["rays"], no_bvh=True), w["got"], "mesh")


def test_closest_area_light_changes_nothing(world, ctx):
    w = world("glass_tri_area")
    assert w["sc"].area_light is not None
    ds = ctx.scene(ss.without_area_light(w["sc"]))
    try:
        assert_outputs_same(ds.closest(w["rays"]), w["got"], "glass_tri_area")
    finally:
        ds.close()


# ------------------------------------------------------------------ sizes, guards, repeats
def _guarded(n):
    """Per output a device buffer of GUARD + n * width + GUARD elements filled with the
    sentinel, and the view of its middle the query writes to."""
    full, view = {}, {}
    for k, width in WIDTH.items():
        if k == "prim":
            full[k] = torch.full((2 * GUARD + n * width,), FILL_I32, dtype=torch.int32, device="cuda")
        else:
            full[k] = torch.full((2 * GUARD + n * width,), FILL, dtype=torch.float64, device="cuda")
        view[k] = full[k][GUARD:GUARD + n * width]
    return full, view


@pytest.mark.parametrize("n", SIZES)
def test_closest_sizes_and_guard_region(ctx, world, n):
    """n around the wave and workgroup sizes, on glass (256-thread workgroups) and on mesh (a
    triangle BVH: one wave per workgroup, the traversal stack in LDS): the device entry writes n
    rows per output, leaves the 64 elements before and after them alone and gives the first n
    rows of the full set's answer; a second call on the same buffers gives the same bytes."""
    for name in ("glass", "mesh"):
        w = world(name)
        d_rays = torch.from_numpy(w["rays"][:n].copy()).cuda()
        full, view = _guarded(n)
        torch.cuda.synchronize()
        first = None
        for _ in range(2):
            res = w["ds"].closest_device(d_rays, capi.CH_ALL, out=view)
            ctx.synchronize()
            raw = {k: full[k].cpu().numpy() for k in WIDTH}
            for k, width in WIDTH.items():
                assert res[k] is view[k]
                fill = FILL_I32 if k == "prim" else FILL
                assert (raw[k][:GUARD] == fill).all() and (raw[k][GUARD + n * width:] == fill).all(), (n, k)
                body = raw[k][GUARD:GUARD + n * width]
                assert_same(body if k == "t" else body.reshape(n, width), w["got"][k][:n], (name, n, k))
            if first is None:
                first = raw
            else:
                assert all(first[k].tobytes() == raw[k].tobytes() for k in WIDTH), n
        assert_outputs_same(w["ds"].closest(w["rays"][:n]), {k: w["got"][k][:n] for k in WIDTH}, (name, n))


# ------------------------------------------------------------------ camera rays
@pytest.fixture(scope="module")
def cam4(ctx):
    """c2 at 24x16 with aa_samples = 4 on the device, and the full frame's rays of samples 0..3."""
    sc = frame_scene("c2")
    ds = ctx.scene(sc)
    rays = [ds.camera_rays(s) for s in range(4)]
    yield dict(sc=sc, ds=ds, rays=rays)
    ds.close()


def test_camera_rays_equal_the_oracle(cam4, oracle):
    sc, ds, rays = cam4["sc"], cam4["ds"], cam4["rays"]
    for s in range(4):
        want = np.array([oracle.get_ray(sc, x, y, aa=s > 0, seed=SEED, sample=s)
                         for y in range(H) for x in range(W)])
        assert_same(rays[s], want, ("sample", s))
    assert_same(rays[0], raysets.camera_rays(sc), "sample 0, unjittered")
    assert (rays[1][:, 3:] != rays[0][:, 3:]).any(axis=1).all()
    assert_same(rays[1][:, :3], rays[0][:, :3], "origins")
    # a second seed changes samples 1..3 and leaves sample 0 alone
    assert_same(ds.camera_rays(0, seed=SEED + 1), rays[0], "seed, sample 0")
    for s in (1, 2, 3):
        other = ds.camera_rays(s, seed=SEED + 1)
        assert (other[:, 3:] != rays[s][:, 3:]).any(axis=1).all(), s
        want = np.array([oracle.get_ray(sc, x, y, aa=True, seed=SEED + 1, sample=s)
                         for y in range(H) for x in range(W)])
        assert_same(other, want, ("second seed", s))


def test_camera_rays_sample_range(cam4):
    ds = cam4["ds"]
    for bad in (-1, 4, 5):
        with pytest.raises(capi.RtError) as e:
            ds.camera_rays(bad)
        assert e.value.status == capi.RT_ERR_INVALID_ARG
    one = ds.cameras([cam4["sc"].camera.position])
    one["aa_samples"] = 1
    assert_same(ds.camera_rays(0, cam=one), cam4["rays"][0], "aa_samples = 1")
    for bad in (1, 2):
        with pytest.raises(capi.RtError):
            ds.camera_rays(bad, cam=one)
        with pytest.raises(capi.RtError):
            ds.camera_rays_device(bad, cam=one)


def _cyclic_rows():
    o = capi.default_opts(**CYCLIC)
    rows = [y for b in range(CYCLIC["row_begin"], H, CYCLIC["row_block"] * CYCLIC["row_cycle"])
            for y in range(b, min(b + CYCLIC["row_block"], H))]
    assert len(rows) == capi.rendered_rows(o, H)
    return rows


def test_camera_rays_row_sets(cam4):
    ds = cam4["ds"]
    for s in (0, 2):
        full = cam4["rays"][s].reshape(H, W, 6)
        assert_same(ds.camera_rays(s, row_begin=3, row_end=11), full[3:11].reshape(-1, 6), "rows")
        assert_same(ds.camera_rays(s, **CYCLIC), full[_cyclic_rows()].reshape(-1, 6), "cyclic")


def test_camera_rays_device_entry_and_guards(cam4, ctx):
    ds = cam4["ds"]
    for s, kw in ((0, {}), (3, {}), (1, dict(row_begin=3, row_end=11)), (2, CYCLIC)):
        host = ds.camera_rays(s, **kw)
        n = len(host)
        full = torch.full((2 * GUARD + 6 * n,), FILL, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        view = full[GUARD:GUARD + 6 * n]
        for _ in range(2):
            res = ds.camera_rays_device(s, out=view, **kw)
            ctx.synchronize()
            assert res is view
            raw = full.cpu().numpy()
            assert (raw[:GUARD] == FILL).all() and (raw[GUARD + 6 * n:] == FILL).all(), (s, kw)
            assert_same(raw[GUARD:GUARD + 6 * n].reshape(n, 6), host, (s, kw))
        own = ds.camera_rays_device(s, **kw)
        ctx.synchronize()
        assert own.shape == (n, 6)
        assert_same(own.cpu().numpy(), host, (s, kw, "own tensor"))


# ------------------------------------------------------------------ trace_rays_device
@pytest.mark.parametrize("name", raysets.GOLDEN_SCENES)
def test_trace_rays_device_equals_the_host_entry(world, ctx, name):
    w = world(name)
    d_rays = torch.from_numpy(w["rays"].copy()).cuda()
    torch.cuda.synchronize()
    for kw in ({}, dict(max_recursion=1), dict(max_recursion=3)):
        got = w["ds"].trace_rays_device(d_rays, **kw)
        ctx.synchronize()
        assert_same(got.cpu().numpy(), w["ds"].trace_rays(w["rays"], **kw), (name, kw))


@pytest.mark.parametrize("n", SIZES)
def test_trace_rays_device_sizes(world, ctx, n):
    w = world("glass")
    want = w["ds"].trace_rays(w["rays"])[:n]
    d_rays = torch.from_numpy(w["rays"][:n].copy()).cuda()
    full = torch.full((2 * GUARD + 3 * n,), FILL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    view = full[GUARD:GUARD + 3 * n]
    assert w["ds"].trace_rays_device(d_rays, out=view) is view
    ctx.synchronize()
    raw = full.cpu().numpy()
    assert (raw[:GUARD] == FILL).all() and (raw[GUARD + 3 * n:] == FILL).all(), n
    assert_same(raw[GUARD:GUARD + 3 * n].reshape(n, 3), want, n)


def test_device_entries_on_a_caller_stream(oracle):
    """On a stream set through rt_context_set_stream the answers are there once that stream has
    synchronised: camera rays, then their trace and their closest hits, without a host copy."""
    sc = frame_scene("glass")
    with capi.Context(0) as c:
        ds = c.scene(sc)
        want_rays = ds.camera_rays(1)
        want_rgb = ds.trace_rays(want_rays)
        want_hit = ds.closest(want_rays)
        stream = torch.cuda.Stream()
        c.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            d_rays = ds.camera_rays_device(1)
            rgb = ds.trace_rays_device(d_rays)
            hit = ds.closest_device(d_rays, capi.CH_T | capi.CH_PRIM)
        stream.synchronize()
        assert_same(d_rays.cpu().numpy(), want_rays, "rays")
        assert_same(rgb.cpu().numpy(), want_rgb, "rgb")
        assert_outputs_same({k: v.cpu().numpy() for k, v in hit.items()},
                            {"t": want_hit["t"], "prim": want_hit["prim"]}, "closest")
        with pytest.raises(ValueError):
            ds.trace_rays_device(d_rays.to(torch.float32))
        with pytest.raises(ValueError):
            ds.closest_device(d_rays, capi.CH_PRIM, out={"prim": torch.zeros(2 * len(want_rays), device="cuda")})
        c.set_stream(None)
        ds.close()


# ------------------------------------------------------------------ the frame from its rays
def _composed(ds, **kw):
    """(Σ_s TraceRay(camera ray of sample s)) / N in GeneratePixelAt's order (Scene.h:289-300),
    on the device."""
    acc = None
    for s in range(4):
        rgb = ds.trace_rays_device(ds.camera_rays_device(s, **kw))
        acc = torch.zeros_like(rgb) if acc is None else acc
        ds.ctx.synchronize()   # torch's stream adds what the context's stream wrote
        acc += rgb
    return (acc / 4.0).cpu().numpy()


@pytest.mark.parametrize("name", ("c2", "glass", "mirror", "c1"))
def test_frame_from_its_rays(ctx, oracle, name):
    """render == (Σ_s trace_rays_device(camera_rays_device(s))) / 4 at 24x16, aa_samples = 4, no
    area light, for the full frame and for the block-cyclic row set: bit for bit on c2 and glass;
    on mirror and c1 to the difference between the parent's rt_render and rt_trace_rays
    (PARENT_RENDER_VS_TRACE), times four."""
    sc = frame_scene(name)
    assert sc.area_light is None
    ds = ctx.scene(sc)
    try:
        for kw in ({}, CYCLIC):
            frame = ds.render(hdr64=True, tonemap=capi.TONEMAP_NONE, **kw)["hdr64"].reshape(-1, 3)
            got = _composed(ds, **kw)
            err = float((np.abs(got - frame) / np.maximum(1.0, np.abs(frame))).max())
            print(f"{name} {kw}: max scaled difference {err:.3e}")
            bar = 4.0 * PARENT_RENDER_VS_TRACE.get(name, 0.0)
            if bar == 0.0:
                assert_same(got, frame, (name, kw))
            else:
                assert err <= bar, (name, kw, err, bar)
    finally:
        ds.close()


# ------------------------------------------------------------------ G-buffer from rays
@pytest.mark.parametrize("name", ("c2", "mesh", "sph300"))
def test_gbuffer_from_rays(ctx, oracle, name):
    """closest_device(camera_rays_device(0)) == the G-buffer's depth, normal and prim; sph300's
    frame sees the sky, so the two miss rules meet there."""
    sc = raysets.scene(name)
    ds = ctx.scene(sc)
    try:
        gb = ds.gbuffer(capi.GB_DEPTH | capi.GB_NORMAL | capi.GB_PRIM)
        hit = ds.closest_device(ds.camera_rays_device(0), capi.CH_T | capi.CH_NORMAL | capi.CH_PRIM)
        ctx.synchronize()
        assert_same(hit["t"].cpu().numpy(), gb["depth"].reshape(-1), (name, "depth"))
        assert_same(hit["normal"].cpu().numpy(), gb["normal"].reshape(-1, 3), (name, "normal"))
        assert_same(hit["prim"].cpu().numpy(), gb["prim"].reshape(-1, 2), (name, "prim"))
        assert np.isfinite(gb["depth"]).sum() >= 100
        assert np.isposinf(gb["depth"]).any() or name != "sph300"
    finally:
        ds.close()


# ------------------------------------------------------------------ shade after hit
@pytest.mark.parametrize("name", ("c2", "mirror"))
def test_shade_after_hit(world, name):
    """closest, then directLightning with the returned material at {point, normal flipped against
    d.normalize(), -d.normalize()} == rt_direct_light_rays on the hit rows: as bits where pow is
    not reached, within 1e-12 * max(1, |ref|) where it is."""
    w = world(name)
    sc, rays, ds, got = w["sc"], w["rays"], w["ds"], w["got"]
    hit = got["prim"][:, 0] != 0
    inc = dl._normalize(rays[hit, 3:])
    n = got["normal"][hit]
    with np.errstate(all="ignore"):
        front = dl._dot(n, inc) < 0.0
    points = np.ascontiguousarray(np.concatenate([got["point"][hit], np.where(front[:, None], n, -n),
                                                  -inc], axis=1))
    mats = np.ascontiguousarray(got["material"][hit])
    assert (mats[:, 5] <= 0.0).all()   # opaque materials
    shaded = ds.direct_light(points, mats)["radiance"]
    ref = ds.direct_light_rays(rays)["radiance"][hit]
    reached = dl.expected(sc, points, mats)["pow"]
    assert_same(shaded[~reached], ref[~reached], (name, "no pow"))
    assert dl.within_bar(shaded, ref).all(), name
    assert (ref != 0.0).any() and (name == "c2") == (not reached.any())


# ------------------------------------------------------------------ C++ drop-in API
def _example_outputs(tmp_path):
    return {"t": np.fromfile(tmp_path / "t.f64", np.float64),
            "prim": np.fromfile(tmp_path / "prim.i32", np.int32).reshape(-1, 2),
            "normal": np.fromfile(tmp_path / "normal.f64", np.float64).reshape(-1, 3),
            "point": np.fromfile(tmp_path / "point.f64", np.float64).reshape(-1, 3),
            "material": np.fromfile(tmp_path / "material.f64", np.float64).reshape(-1, 7)}


def test_cpp_closest_scenefile(world, ctx, tmp_path):
    """examples/closest_scenefile: Scene::IntersectClosest(rays) gives the Python call's bytes
    for a rays file, and with --camera 1 Scene::CameraRays(1) and their hits do."""
    w = world("glass")
    scene = tmp_path / "scene.txt"
    w["sc"].write(scene)
    w["rays"].tofile(tmp_path / "rays_in.f64")
    run = subprocess.run([EXE, str(scene), str(tmp_path / "rays_in.f64"), str(tmp_path)],
                         check=True, capture_output=True, text=True, timeout=120)
    assert len(run.stdout.splitlines()) == len(w["rays"])
    assert_outputs_same(_example_outputs(tmp_path), w["got"], "rays file")

    sc = frame_scene("glass")
    sc.write(scene)
    ds = ctx.scene(sc)
    try:
        rays = ds.camera_rays(1)
        want = ds.closest(rays)
    finally:
        ds.close()
    run = subprocess.run([EXE, "--camera", "1", str(scene), str(tmp_path)], check=True,
                         capture_output=True, text=True, timeout=120)
    assert len(run.stdout.splitlines()) == W * H
    assert_same(np.fromfile(tmp_path / "rays.f64", np.float64).reshape(-1, 6), rays, "camera rays")
    assert_outputs_same(_example_outputs(tmp_path), want, "--camera 1")
    line = run.stdout.splitlines()[5].split()
    assert line[0] == "5" and float(line[2]) == want["t"][5] and int(line[4]) == want["prim"][5, 0]
