"""rt_scatter_rays and rt_scatter_rays_device (rt_scatter.hip): one level of Scene::TraceRay
(Scene.h:131-198) per ray, before its children are traced, on the 648-ray sets of
tests/raysets.py.

The comparator is the table of tests/scatter_sets.py: a numpy restatement of the level which,
applied level by level, equals the oracle's TraceRay bit for bit (tests/test_oracle_scatter.py).
Flags, child rays and a miss's value are compared as bits; a hit's value as bits where
directLightning does not reach std::pow and within 1e-12 * max(1, |ref|) where it does; the
weights as bits on opaque materials and within the same bar on transparent ones, whose weights
pass through the Fresnel pow."""
import os
import subprocess

import numpy as np
import pytest
import torch

import direct_light_sets as dl
import raysets
import scatter_sets as ss
from raytracingengine_amd import capi
from raytracingengine_amd.scene import SceneData

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "bin", "scatter_scenefile")
SIZES = (0, 1, 63, 64, 65, 255, 256, 257)
GUARD = 64
FILL = -7.25          # the guard value of the float64 outputs: no colour, no ray, no weight
FILL_U8 = 0xA5        # and of the flags: no flags byte (those are <= 7)
WIDTH = {"value": 3, "refract_rays": 6, "reflect_rays": 6, "weights": 2, "flags": 1}
BITS = {"value": capi.SC_VALUE, "refract_rays": capi.SC_REFRACT, "reflect_rays": capi.SC_REFLECT,
        "weights": capi.SC_WEIGHTS, "flags": capi.SC_FLAGS}


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


def assert_table(got, t, what, rows=slice(None)):
    """got: the dict of an SC_ALL call; t: a table of scatter_sets (or the rows `rows` of it)."""
    flags = t["flags"][rows]
    assert_same(got["flags"], flags, (what, "flags"))
    assert_same(got["refract_rays"], t["refract_rays"][rows], (what, "refract_rays"))
    assert_same(got["reflect_rays"], t["reflect_rays"][rows], (what, "reflect_rays"))
    hit = (flags & ss.HIT) != 0
    # a miss: the sky bit for bit; a hit: bits where directLightning does not reach pow
    exact = ~hit | ~t["pow_value"][rows]
    ref = t["value"][rows]
    assert got["value"].shape == ref.shape and got["value"].dtype == np.float64, what
    assert_same(got["value"][exact], ref[exact], (what, "value, no pow"))
    ok = dl.within_bar(got["value"], ref)
    err = np.abs(got["value"] - ref) / np.maximum(1.0, np.abs(ref))
    assert ok.all(), (what, "value", np.argwhere(~ok)[:4], float(np.nanmax(err)))
    # weights: the material's specular bit for bit on opaque hits, through pow on transparent ones
    fres = t["fresnel"][rows]
    ref = t["weights"][rows]
    assert got["weights"].shape == ref.shape and got["weights"].dtype == np.float64, what
    assert_same(got["weights"][~fres], ref[~fres], (what, "weights, opaque"))
    ok = dl.within_bar(got["weights"], ref)
    err = np.abs(got["weights"] - ref) / np.maximum(1.0, np.abs(ref))
    assert ok.all(), (what, "weights", np.argwhere(~ok)[:4], float(np.nanmax(err)))
    tir = t["tir"][rows]
    assert (got["weights"][tir, 1] == 1.0).all() and not bits(got["weights"][tir, 0]).any(), what
    # an absent child: all-zero bits, rays and weight
    for key, bit, w in (("refract_rays", ss.REFRACT, 0), ("reflect_rays", ss.REFLECT, 1)):
        gone = (got["flags"] & bit) == 0
        assert not bits(got[key][gone]).any() and not bits(got["weights"][gone, w]).any(), (what, key)
    assert not bits(got["weights"][~hit]).any(), what


@pytest.fixture(scope="module")
def world(ctx, oracle):
    """Per scene, made once and left unchanged: the table, the scene on the device (with its
    area light, where it has one) and the device's SC_ALL answer."""
    cache = {}

    def get(name):
        if name not in cache:
            t = ss.scene_set(name)
            ds = ctx.scene(t["sc"])
            cache[name] = dict(t=t, ds=ds, got=ds.scatter(t["rays"]))
        return cache[name]
    yield get
    for w in cache.values():
        w["ds"].close()


# ------------------------------------------------------------------ values
@pytest.mark.parametrize("name", ss.SCENES)
def test_tables(world, name):
    w = world(name)
    t, got = w["t"], w["got"]
    assert got["flags"].dtype == np.uint8 and got["flags"].shape == (len(t["rays"]),)
    assert_table(got, t, name)
    hit = (got["flags"] & 1) != 0
    assert_same(got["value"][~hit], ss.sky(t["rays"])[~hit], (name, "sky"))
    assert hit.sum() >= 100 and (~hit).sum() >= 1
    # the copies of ray 0 give ray 0's rows
    for i in raysets.repeat_indices(len(t["rays"])):
        for k in ss.OUTPUTS:
            assert got[k][i].tobytes() == got[k][0].tobytes(), (name, k, i)


@pytest.mark.parametrize("name,depth", (("glass", 3), ("mirror", 4), ("c2", 2)))
def test_recomposition_on_the_device(world, oracle, name, depth):
    """capi.compose_trace — scatter level by level, the children selected by the flags, terminal
    at `depth` — against rt_trace_rays with max_recursion = depth and against the oracle's
    TraceRay: bit for bit on c2 (no pow, no children), else within 1e-12 * max(1, |v|) (the
    chain kernels accumulate front to back)."""
    w = world(name)
    rays, ds = w["t"]["rays"], w["ds"]
    composed = capi.compose_trace(ds, rays, depth)
    traced = ds.trace_rays(rays, max_recursion=depth)
    ref, _, _ = oracle.trace_rays(w["t"]["sc"], rays, max_recursion=depth, use_area_light=False)
    assert composed.shape == traced.shape == ref.shape and np.isfinite(ref).all()
    for other, tag in ((traced, "rt_trace_rays"), (ref, "oracle")):
        err = np.abs(composed - other) / np.maximum(1.0, np.abs(other))
        print(f"{name} depth {depth} vs {tag}: max scaled error {err.max():.3e}, "
              f"bit-equal rays {100.0 * (bits(composed) == bits(other)).all(axis=1).mean():.1f} %")
        if name == "c2":
            assert_same(composed, other, (name, tag))
        else:
            assert dl.within_bar(composed, other).all(), (name, tag, float(err.max()))
    if name != "c2":    # the children matter: the level alone is not the answer
        assert not dl.within_bar(w["got"]["value"], ref).all()


@pytest.mark.parametrize("name", ("c2", "glass", "mirror", "mesh"))
def test_consistent_with_the_other_queries(world, name):
    """On the same rays: value == direct_light_rays' radiance * (1 - clamp(transparency)) formed
    in numpy with the hit primitive's material, bit for bit on hit rows; flags & 1 is
    intersect_rays' type != 0."""
    w = world(name)
    t, ds, got = w["t"], w["ds"], w["got"]
    cl = ds.intersect_rays(t["rays"])
    hit = cl[:, 0] != 0
    assert np.array_equal((got["flags"] & 1) != 0, hit)
    rad = ds.direct_light_rays(t["rays"], capi.DL_RADIANCE)["radiance"][hit]
    tables = dl.scene_materials(t["sc"])
    tr = np.zeros(int(hit.sum()))
    for k in (1, 2, 3):
        sel = cl[hit, 0] == k
        if sel.any():
            tr[sel] = tables[k - 1][cl[hit][sel, 1].astype(np.int64), 5]
    tr = np.where(tr < 0.0, 0.0, np.where(1.0 < tr, 1.0, tr))
    want = np.where((tr < 1.0)[:, None], np.zeros((len(tr), 3)) + rad * (1.0 - tr)[:, None], 0.0)
    assert_same(got["value"][hit], want, name)
    assert (want != 0.0).any()


# ------------------------------------------------------------------ output subsets
@pytest.mark.parametrize("name", ("glass", "c2"))
def test_terminal_is_all_sky(world, name):
    w = world(name)
    rays = w["t"]["rays"]
    got = w["ds"].scatter(rays, terminal=True)
    assert_same(got["value"], ss.sky(rays), (name, "sky"))
    assert not got["flags"].any()
    for k in ("refract_rays", "reflect_rays", "weights"):
        assert got[k].shape == (len(rays), WIDTH[k]) and not bits(got[k]).any(), k
    assert_outputs_same(got, {k: ss.level(w["t"]["sc"], rays, terminal=True)[k] for k in ss.OUTPUTS},
                        (name, "restatement"))
    only = w["ds"].scatter(rays, outputs=capi.SC_VALUE, terminal=True)
    assert_outputs_same(only, {"value": got["value"]}, (name, "value alone"))


@pytest.mark.parametrize("name", ("glass", "mirror", "c2"))
def test_output_subsets_equal_the_full_call(world, name):
    """Each single output bit, VALUE|FLAGS, and all but VALUE: the slice of SC_ALL bit for bit
    (the kernel's DIRECT and CHILDREN instances agree)."""
    w = world(name)
    rays, full = w["t"]["rays"], w["got"]
    subsets = [b for b in BITS.values()] + [capi.SC_VALUE | capi.SC_FLAGS, capi.SC_ALL & ~capi.SC_VALUE]
    for outputs in subsets:
        got = w["ds"].scatter(rays, outputs=outputs)
        want = {k: full[k] for k, b in BITS.items() if outputs & b}
        assert_outputs_same(got, want, (name, hex(outputs)))
    for bad in (0, 0x20, 0x3f):
        with pytest.raises(ValueError):
            w["ds"].scatter(rays, outputs=bad)


def test_area_light_is_not_read(world, ctx):
    """glass_tri_area with its area light attached equals the same scene without it."""
    w = world("glass_tri_area")
    assert w["t"]["sc"].area_light is not None
    ds = ctx.scene(ss.without_area_light(w["t"]["sc"]))
    try:
        assert_outputs_same(ds.scatter(w["t"]["rays"]), w["got"], "glass_tri_area")
    finally:
        ds.close()


@pytest.mark.parametrize("name", ("mesh", "bigmesh"))
def test_no_bvh_equals_bvh(world, name):
    w = world(name)
    assert_outputs_same(w["ds"].scatter(w["t"]["rays"], no_bvh=True), w["got"], name)


def test_bias_is_read(world):
    """bias = 1e-2 gives the table made with that bias, whose child origins differ."""
    t = ss.scene_set("glass", 1e-2)
    got = world("glass")["ds"].scatter(t["rays"], bias=1e-2)
    assert_table(got, t, "glass bias 1e-2")
    assert not dl.same_bits(got["reflect_rays"], world("glass")["got"]["reflect_rays"])


# ------------------------------------------------------------------ sizes, guards, repeats
def _guarded(n):
    """Per output a device buffer of GUARD + n * width + GUARD elements filled with the
    sentinel, and the view of its middle the query writes to."""
    full, view = {}, {}
    for k, width in WIDTH.items():
        if k == "flags":
            full[k] = torch.full((2 * GUARD + n,), FILL_U8, dtype=torch.uint8, device="cuda")
        else:
            full[k] = torch.full((2 * GUARD + n * width,), FILL, dtype=torch.float64, device="cuda")
        view[k] = full[k][GUARD:GUARD + n * width]
    return full, view


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_guard_region(ctx, world, n):
    """n around the wave and workgroup sizes: the host entry gives the table's first n rows; the
    device entry writes n rows per output and leaves the 64 elements before and after them
    alone; a second call on the same buffers gives the same bytes."""
    w = world("glass")
    t, ds = w["t"], w["ds"]
    rays = t["rays"][:n]
    host = ds.scatter(rays)
    assert_table(host, t, n, slice(0, n))
    assert_outputs_same(host, {k: w["got"][k][:n] for k in ss.OUTPUTS}, n)
    d_rays = torch.from_numpy(rays.copy()).cuda()
    full, view = _guarded(n)
    torch.cuda.synchronize()
    first = None
    for _ in range(2):
        res = ds.scatter_device(d_rays, out=view)
        ctx.synchronize()
        raw = {k: full[k].cpu().numpy() for k in WIDTH}
        for k, width in WIDTH.items():
            assert res[k] is view[k]
            fill = FILL_U8 if k == "flags" else FILL
            assert (raw[k][:GUARD] == fill).all() and (raw[k][GUARD + n * width:] == fill).all(), (n, k)
            body = raw[k][GUARD:GUARD + n * width]
            assert_same(body if k == "flags" else body.reshape(n, width), host[k], (n, k))
        if first is None:
            first = raw
        else:
            assert all(first[k].tobytes() == raw[k].tobytes() for k in WIDTH), n


def test_buffer_grows_and_shrinks(oracle):
    """ctx->rays (6 doubles per ray, 113 bytes per ray of outputs) grows on demand: growing and
    shrinking n and the output set on one fresh context gives the table each time."""
    t = ss.scene_set("mirror")
    with capi.Context(0) as c:
        ds = c.scene(t["sc"])
        for n, outputs in ((3, capi.SC_ALL), (len(t["rays"]), capi.SC_ALL), (65, capi.SC_FLAGS),
                           (257, capi.SC_REFLECT | capi.SC_FLAGS), (1, capi.SC_ALL)):
            got = ds.scatter(t["rays"][:n], outputs=outputs)
            if outputs == capi.SC_ALL:
                assert_table(got, t, n, slice(0, n))
            else:
                assert_outputs_same(got, {k: t[k][:n] for k, b in BITS.items() if outputs & b}, n)
            ds.intersect_rays(t["rays"][:max(1, n // 2)])
        ds.close()


# ------------------------------------------------------------------ device tensors, streams
def test_device_entry_on_a_caller_stream(oracle):
    """On a stream set through rt_context_set_stream the answers are there once that stream has
    synchronised."""
    t = ss.scene_set("glass")
    with capi.Context(0) as c:
        ds = c.scene(t["sc"])
        stream = torch.cuda.Stream()
        c.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            d_rays = torch.from_numpy(t["rays"].copy()).to("cuda", non_blocking=False)
            a = ds.scatter_device(d_rays)
            b = ds.scatter_device(d_rays, outputs=capi.SC_VALUE | capi.SC_FLAGS)
        stream.synchronize()
        got = {k: v.cpu().numpy() for k, v in a.items()}
        assert_table(got, t, "glass stream")
        assert_outputs_same({k: v.cpu().numpy() for k, v in b.items()},
                            {"value": got["value"], "flags": got["flags"]}, "glass stream subset")
        with pytest.raises(ValueError):
            ds.scatter_device(d_rays.to(torch.float32))
        with pytest.raises(ValueError):
            ds.scatter_device(d_rays, out={"flags": torch.zeros(len(t["rays"]), device="cuda")})
        c.set_stream(None)
        ds.close()


# ------------------------------------------------------------------ no lights, empty scene
def test_scene_without_lights_and_empty_scene(ctx, oracle):
    """Without lights an opaque hit's value is zero and the mirrors still have their reflection
    rays; in an empty scene every ray is a miss: the sky."""
    t = ss.scene_set("mirror")
    sc = t["sc"]
    dark = SceneData(sc.camera, sc.spheres, sc.planes, sc.triangles, sc.models)
    ds = ctx.scene(dark)
    try:
        got = ds.scatter(t["rays"])
        hit = (got["flags"] & 1) != 0
        assert not bits(got["value"][hit]).any() and hit.sum() >= 300
        for k in ("flags", "reflect_rays", "refract_rays", "weights"):
            assert_same(got[k], t[k], ("dark", k))
        assert ((got["flags"] & ss.REFLECT) != 0).sum() >= 500
        assert_table(got, ss.level(dark, t["rays"]), "dark")
    finally:
        ds.close()
    ds = ctx.scene(SceneData(sc.camera))
    try:
        got = ds.scatter(t["rays"])
        assert_outputs_same(got, {k: ss.level(sc, t["rays"], terminal=True)[k] for k in ss.OUTPUTS},
                            "empty")
        assert ds.scatter(np.empty((0, 6)))["weights"].shape == (0, 2)
        assert ds.scatter(np.empty((0, 6)))["flags"].shape == (0,)
    finally:
        ds.close()


# ------------------------------------------------------------------ non-finite inputs
@pytest.mark.parametrize("name", ("c2", "glass", "mesh", "glass_tri_area"))
def test_nonfinite_rays(world, name):
    """Zero, NaN, infinite, huge and denormal o and d: the call returns, flags <= 7, the finite
    rays in between have their table rows, and where the oracle's IntersectClosest reports a hit
    the hit bit is set and the children are the restatement's (NaNs where it has NaNs)."""
    w = world(name)
    sc = w["t"]["sc"]
    rays = raysets.nonfinite_rays(sc)
    e = ss.level(sc, rays)
    got = w["ds"].scatter(rays)
    assert got["flags"].shape == (len(rays),) and (got["flags"] <= 7).all()
    finite = np.flatnonzero((rays == rays[2]).all(axis=1))   # the ordinary ray, three times
    assert len(finite) == 3 and np.isfinite(rays[2]).all()
    assert_table({k: got[k][finite] for k in ss.OUTPUTS}, {k: v[finite] for k, v in e.items()},
                 (name, "finite rows"))
    hit = (e["flags"] & ss.HIT) != 0
    assert ((got["flags"][hit] & 1) != 0).all(), name
    assert np.array_equal(got["flags"][hit], e["flags"][hit]), (name, got["flags"][hit], e["flags"][hit])
    for k in ("refract_rays", "reflect_rays"):
        a, b = dl.canonical_bits(got[k][hit]), dl.canonical_bits(e[k][hit])
        assert np.array_equal(a, b), (name, k, np.argwhere(a != b)[:4])


# ------------------------------------------------------------------ C++ drop-in API
@pytest.mark.parametrize("name,depth", (("c2", 2), ("glass", 3)))
def test_cpp_scatter_rays(world, tmp_path, name, depth):
    """examples/scatter_scenefile: Scene::ScatterRays gives the Python call's bytes, and its
    composition to `depth` the bytes of capi.compose_trace; Scene::TraceRays those of
    trace_rays."""
    w = world(name)
    t, got = w["t"], w["got"]
    scene = tmp_path / "scene.txt"
    t["sc"].write(scene)
    t["rays"].tofile(tmp_path / "rays.f64")
    run = subprocess.run([EXE, "--depth", str(depth), str(scene), str(tmp_path / "rays.f64"),
                          str(tmp_path)], check=True, capture_output=True, text=True, timeout=120)
    assert len(run.stdout.splitlines()) == 2 * len(t["rays"])

    def load(stem, width):
        return np.fromfile(tmp_path / f"{stem}.f64", np.float64).reshape(-1, width)
    assert_same(load("value", 3), got["value"], (name, "value"))
    assert_same(load("refraction", 6), got["refract_rays"], (name, "refraction"))
    assert_same(load("reflection", 6), got["reflect_rays"], (name, "reflection"))
    assert_same(load("weights", 2), got["weights"], (name, "weights"))
    assert_same(np.fromfile(tmp_path / "flags.u8", np.uint8), got["flags"], (name, "flags"))
    assert_same(load("composed", 3), capi.compose_trace(w["ds"], t["rays"], depth), (name, "composed"))
    assert_same(load("traced", 3), w["ds"].trace_rays(t["rays"], max_recursion=depth), (name, "traced"))
