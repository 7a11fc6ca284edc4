"""rt_direct_light / rt_direct_light_rays and their _device variants (rt_direct.hip): the batch
Scene::directLightning (Scene.h:79-129) for caller-supplied surface points and for the first hits
of rays, on the ray sets of tests/raysets.py.

The comparator is the table of tests/direct_light_sets.py: a numpy restatement of the reference's
light loop with one oracle_transmittance call per shadow ray, held against the oracle's TraceRay
in tests/test_oracle_direct_light.py.  Diffuse is compared as float64 bits everywhere; specular
and radiance as bits where std::pow is not reached and within 1e-12 * max(1, |ref|) where it is
(the project's bar for values that pass through pow)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import direct_light_sets as dl
import raysets
import transmittance_sets as ts
from raytracingengine_amd import capi
from raytracingengine_amd.scene import SceneData

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "bin", "direct_light_scenefile")
SIZES = (0, 1, 63, 64, 65, 255, 256, 257)
GUARD = 64
FILL = -7.25          # the guard value: no radiance
NAMES = ("radiance", "diffuse", "specular")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.flatnonzero((bits(got) != bits(want)).reshape(len(got), -1).any(axis=1)) if got.size else []
    assert not len(bad), (what, len(bad), bad[:8], got[bad[:4]], want[bad[:4]])


def assert_table(got, e, what, rows=slice(None)):
    """got: the dict of a DL_ALL call; e: a table of direct_light_sets (or a slice of it)."""
    pw = e["pow"][rows]
    assert_same(got["diffuse"], e["diffuse"][rows], (what, "diffuse"))
    for k in ("specular", "radiance"):
        ref = e[k][rows]
        assert got[k].shape == ref.shape and got[k].dtype == np.float64, (what, k)
        assert_same(got[k][~pw], ref[~pw], (what, k, "no pow"))
        ok = dl.within_bar(got[k], ref)
        err = np.abs(got[k] - ref) / np.maximum(1.0, np.abs(ref))
        assert ok.all(), (what, k, np.argwhere(~ok)[:4], float(np.nanmax(err)))


def assert_composed(got, materials, what):
    """radiance == color * diffuse + specular * material.specular, bit for bit, formed from the
    call's own diffuse and specular outputs."""
    m = np.broadcast_to(np.asarray(materials, np.float64).reshape(-1, 7), (len(got["diffuse"]), 7))
    with np.errstate(all="ignore"):
        want = m[:, :3] * got["diffuse"] + got["specular"] * m[:, 4:5]
    assert np.array_equal(dl.canonical_bits(got["radiance"]), dl.canonical_bits(want)), what


def points_of_rays(ds, sc, rays, **kw):
    """The points entry on the oracle's hits of `rays`, scattered to one row per ray (+0.0 where
    the ray misses): what the rays entry must give."""
    h = dl.hits(sc, rays)
    got = ds.direct_light(h["points"], h["materials"], capi.DL_ALL, **kw)
    out = {}
    for k in NAMES:
        out[k] = np.zeros((len(rays), 3), np.float64)
        out[k][h["index"]] = got[k]
    return h, out


# ------------------------------------------------------------------ values: the points entry
@pytest.mark.parametrize("name", dl.LIGHT_SCENES)
def test_points_tables(ctx, oracle, name):
    """Hit points of the scene's ray set (and every fourth again from behind) with the hit
    primitives' materials; on c3 and c4, whose materials have no specular, once more with
    caller-supplied specular materials."""
    for own in (True, False) if name in dl.SPEC_SCENES else (True,):
        s = dl.scene_set(name, own_materials=own)
        ds = ctx.scene(s["sc"])
        try:
            got = ds.direct_light(s["points"], s["materials"], capi.DL_ALL)
            assert_table(got, s, (name, own))
            assert_composed(got, s["materials"], (name, own))
            if not own:
                assert (got["specular"] != 0.0).any()
        finally:
            ds.close()


def test_points_row_of_glass(ctx, oracle):
    """The T <= bias drop (Scene.h:105) and the shared-material form on the crafted row."""
    r = dl.row_set()
    ds = ctx.scene(r["sc"])
    try:
        got = ds.direct_light(r["points"], r["materials"], capi.DL_ALL)
        assert_table(got, r, "row")
        assert_composed(got, r["materials"], "row")
    finally:
        ds.close()


def test_bias_is_read(ctx, oracle):
    """bias = 1e-2 gives the table made with that bias, which differs from the one at 1e-3: on
    the crafted row the point behind four spheres (T = 0.5^8 = 3.9e-3) loses its first light."""
    a, b = dl.row_set(1e-2), dl.row_set()
    assert not dl.same_bits(a["diffuse"], b["diffuse"])
    ds = ctx.scene(a["sc"])
    try:
        got = ds.direct_light(a["points"], a["materials"], capi.DL_ALL, bias=1e-2)
        assert_table(got, a, "row bias 1e-2")
        assert not dl.same_bits(got["diffuse"], b["diffuse"])
    finally:
        ds.close()
    g = dl.scene_set("glass", 1e-2)
    ds = ctx.scene(g["sc"])
    try:
        got = ds.direct_light(g["points"], g["materials"], capi.DL_ALL, bias=1e-2)
        assert_table(got, g, "glass bias 1e-2")
        rays = ds.direct_light_rays(g["rays"], capi.DL_DIFFUSE, bias=1e-2)["diffuse"]
        assert_same(rays[g["index"]], g["diffuse"][:g["n_hits"]], "glass rays bias 1e-2")
    finally:
        ds.close()


# ------------------------------------------------------------------ values: the rays entry
@pytest.mark.parametrize("name", list(raysets.SCENES))
def test_rays_equal_points_on_the_oracles_hits(ctx, oracle, name):
    """Per ray: IntersectClosest, the normal flip and the view of TraceRay, the hit primitive's
    material — the bits of the points entry fed the oracle's hits; a miss is +0.0 in every
    output.  On the scenes where TraceRay is directLightning at the hit, the oracle's TraceRay."""
    sc = raysets.scene(name)
    rays, _ = raysets.rayset(sc)
    if len(sc.triangle_array()) > ts.MESH_TRIS:
        rays = rays[:2 * ts.MESH_RAYS]
    ds = ctx.scene(sc)
    try:
        got = ds.direct_light_rays(rays, capi.DL_ALL)
        h, want = points_of_rays(ds, sc, rays)
        miss = np.setdiff1d(np.arange(len(rays)), h["index"])
        assert len(h["index"]) >= 100
        for k in NAMES:
            assert_same(got[k], want[k], (name, k))
            assert not bits(got[k][miss]).any(), (name, k, "a miss is not +0.0")
        assert_composed({k: got[k][h["index"]] for k in NAMES}, h["materials"], name)
        if name in dl.DIRECT_SCENES:
            ref, _, _ = oracle.trace_rays(sc, rays[h["index"]])
            assert (got["radiance"][h["index"]] == ref).all(), name
            assert (ref != 0.0).any()
        if sc.area_light is not None:      # the area light is not read
            bare = SceneData(sc.camera, sc.spheres, sc.planes, sc.triangles, sc.models, sc.lights)
            db = ctx.scene(bare)
            try:
                again = db.direct_light_rays(rays, capi.DL_ALL)
            finally:
                db.close()
            for k in NAMES:
                assert_same(again[k], got[k], (name, k, "area light detached"))
    finally:
        ds.close()


@pytest.mark.parametrize("name", ["c2", "glass", "mesh"])
def test_rays_tables(ctx, oracle, name):
    """The rays entry against the CPU table directly."""
    s = dl.scene_set(name)
    ds = ctx.scene(s["sc"])
    try:
        got = ds.direct_light_rays(s["rays"], capi.DL_ALL)
        assert_table({k: got[k][s["index"]] for k in NAMES}, s, name, slice(0, s["n_hits"]))
    finally:
        ds.close()


# ------------------------------------------------------------------ variants
def test_shared_material_equals_repeated(ctx, oracle):
    s = dl.scene_set("c3", own_materials=False)
    ds = ctx.scene(s["sc"])
    try:
        for row in (1, 2, 9):      # opaque specular, another shininess, transparent
            one = s["materials"][row]
            n = len(s["points"])
            rep = ds.direct_light(s["points"], np.tile(one, (n, 1)), capi.DL_ALL)
            shared = ds.direct_light(s["points"], one, capi.DL_ALL)
            for k in NAMES:
                assert_same(shared[k], rep[k], ("shared", row, k))
            d_pts = torch.from_numpy(s["points"].copy()).cuda()
            d_mat = torch.from_numpy(np.tile(one, (n, 1))).cuda()
            torch.cuda.synchronize()
            a = ds.direct_light_device(d_pts, tuple(one), capi.DL_ALL)
            b = ds.direct_light_device(d_pts, d_mat, capi.DL_ALL)
            ctx.synchronize()
            for k in NAMES:
                assert_same(a[k].cpu().numpy(), rep[k], ("shared device", row, k))
                assert_same(b[k].cpu().numpy(), rep[k], ("per point device", row, k))
        assert (rep["specular"] == 0.0).all() and (shared["diffuse"] != 0.0).any()   # row 9
    finally:
        ds.close()


def test_single_outputs_equal_slices_of_all(ctx, oracle):
    """Each single bit gives the matching output of RT_DL_ALL, and the pointers of outputs that
    were not requested are not written through."""
    s = dl.scene_set("glass")
    ds = ctx.scene(s["sc"])
    lib = capi.load_library()
    try:
        every = ds.direct_light(s["points"], s["materials"], capi.DL_ALL)
        every_r = ds.direct_light_rays(s["rays"], capi.DL_ALL)
        for name, bit in capi.DL_OUTPUTS:
            one = ds.direct_light(s["points"], s["materials"], bit)
            assert list(one) == [name]
            assert_same(one[name], every[name], name)
            one = ds.direct_light_rays(s["rays"], bit)
            assert list(one) == [name]
            assert_same(one[name], every_r[name], name)
        assert list(ds.direct_light_rays(s["rays"])) == ["radiance"]
        n = len(s["rays"])
        d_rays = torch.from_numpy(s["rays"].copy()).cuda()
        want = torch.full((3 * n,), FILL, dtype=torch.float64, device="cuda")
        other = torch.full((3 * n,), FILL, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ptrs = capi.DirectLightPtrs(other.data_ptr(), want.data_ptr(), other.data_ptr())
        o = capi.default_opts()
        assert lib.rt_direct_light_rays_device(ctx.handle, ds._h, ctypes.byref(o), d_rays.data_ptr(),
                                               n, capi.DL_DIFFUSE, ctypes.byref(ptrs)) == capi.RT_OK
        ctx.synchronize()
        assert (other.cpu().numpy() == FILL).all()
        assert_same(want.cpu().numpy().reshape(n, 3), every_r["diffuse"], "diffuse alone")
        with pytest.raises(ValueError):
            ds.direct_light_rays(s["rays"], 0)
        with pytest.raises(ValueError):
            ds.direct_light_rays(s["rays"], 0x8)
    finally:
        ds.close()


@pytest.mark.parametrize("name", ts.BVH_SCENES + ts.BVH_GRIDS)
def test_bvh_equals_every_triangle(ctx, oracle, name):
    if name in ts.BVH_GRIDS:
        sc, rays, _ = raysets.CRAFTED[name]()
    else:
        sc = raysets.scene(name)
        rays = raysets.rayset(sc)[0][:2 * ts.MESH_RAYS]
    assert len(sc.triangle_array()) >= 32       # a BVH is built
    ds = ctx.scene(sc)
    try:
        a = ds.direct_light_rays(rays, capi.DL_ALL)
        b = ds.direct_light_rays(rays, capi.DL_ALL, no_bvh=True)
        h, pa = points_of_rays(ds, sc, rays)
        _, pb = points_of_rays(ds, sc, rays, no_bvh=True)
        for k in NAMES:
            assert_same(b[k], a[k], (name, k))
            assert_same(pb[k], pa[k], (name, k, "points"))
            assert_same(a[k], pa[k], (name, k, "rays against points"))
        e = dl.expected(sc, h["points"], h["materials"])
        assert_table({k: a[k][h["index"]] for k in NAMES}, e, name)
        assert (a["diffuse"] != 0.0).any()
    finally:
        ds.close()


CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import direct_light_sets as dl
import raysets
import transmittance_sets as ts
from raytracingengine_amd import capi
out = {}
with capi.Context(0) as c:
    for name in ts.OPAQUE_SCENES:
        sc = raysets.scene(name)
        rays = raysets.rayset(sc)[0]
        h = dl.hits(sc, rays)
        ds = c.scene(sc)
        for k, v in ds.direct_light_rays(rays, capi.DL_ALL).items():
            out[f"{name}_rays_{k}"] = v
        for k, v in ds.direct_light(h["points"], h["materials"], capi.DL_ALL).items():
            out[f"{name}_points_{k}"] = v
        ds.close()
np.savez(sys.argv[3], **out)
"""


def test_opaque_fast_path_equals_the_march(oracle, tmp_path):
    """RTAMD_TX_OPAQUE=0 (the exact march alone) against the default (occlusion_opaque first) on
    the scenes without transparency, each setting in a fresh process: the same bits."""
    res = {}
    for tag, val in (("default", None), ("march", "0")):
        env = dict(os.environ)
        env.pop("RTAMD_TX_OPAQUE", None)
        if val is not None:
            env["RTAMD_TX_OPAQUE"] = val
        path = tmp_path / f"{tag}.npz"
        subprocess.run([sys.executable, "-c", CHILD, ROOT, os.path.join(ROOT, "tests"), str(path)],
                       check=True, env=env, timeout=300)
        res[tag] = dict(np.load(path))
    assert set(res["default"]) == set(res["march"]) and len(res["default"]) == 6 * len(ts.OPAQUE_SCENES)
    for key, v in res["default"].items():
        assert raysets.SCENES[key.split("_")[0]]["path"] != "tree"      # no transparent material
        assert_same(v, res["march"][key], key)
    s = dl.scene_set("c2")
    assert_same(res["default"]["c2_rays_diffuse"][s["index"]], s["diffuse"][:s["n_hits"]], "c2")
    assert (res["default"]["mesh_points_specular"] != 0.0).any()


# ------------------------------------------------------------------ sizes, guards, repeats
@pytest.fixture(scope="module")
def c4(ctx, oracle):
    s = dl.scene_set("c4", own_materials=False)
    ds = ctx.scene(s["sc"])
    yield ds, s
    ds.close()


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_guard_region(ctx, c4, n):
    """n around the wave and workgroup sizes: the host entries give the tables' first n rows; the
    device entries write n * 3 doubles per output and leave the 64 after them alone; a second
    call gives the same bits."""
    ds, s = c4
    pts, mats = s["points"][:n], s["materials"][:n]
    rays = s["rays"][:n]
    got = ds.direct_light(pts, mats, capi.DL_ALL)
    assert_table(got, s, n, slice(0, n))
    host_rays = ds.direct_light_rays(rays, capi.DL_ALL)
    d_pts = torch.from_numpy(pts.copy()).cuda()
    d_mat = torch.from_numpy(mats.copy()).cuda()
    d_rays = torch.from_numpy(rays.copy()).cuda()
    outs = [{k: torch.full((3 * n + GUARD,), FILL, dtype=torch.float64, device="cuda") for k in NAMES}
            for _ in range(2)]
    torch.cuda.synchronize()
    for _ in range(2):
        if n == 1:      # one row of materials is the shared form: a host record
            res_p = ds.direct_light_device(d_pts, mats[0], capi.DL_ALL, out=outs[0])
        else:
            res_p = ds.direct_light_device(d_pts, d_mat, capi.DL_ALL, out=outs[0])
        res_r = ds.direct_light_rays_device(d_rays, capi.DL_ALL, out=outs[1])
        ctx.synchronize()
        for k in NAMES:
            assert res_p[k] is outs[0][k] and res_r[k] is outs[1][k]
            hp, hr = outs[0][k].cpu().numpy(), outs[1][k].cpu().numpy()
            assert (hp[3 * n:] == FILL).all() and (hr[3 * n:] == FILL).all(), (n, k)
            assert_same(hp[:3 * n].reshape(n, 3), got[k], (n, k, "points"))
            assert_same(hr[:3 * n].reshape(n, 3), host_rays[k], (n, k, "rays"))


def test_buffer_grows_and_shrinks(oracle):
    """ctx->rays (16 + 9 doubles per point here, 6 + 9 per ray) grows on demand: growing and
    shrinking n on one fresh context, with the other batch entries in between, gives the tables
    each time."""
    s = dl.scene_set("mesh")
    t = ts.scene_table("mesh")
    with capi.Context(0) as c:
        ds = c.scene(s["sc"])
        for n in (3, 700, 64, len(s["points"]), 1, 257):
            n = min(n, len(s["points"]))
            got = ds.direct_light(s["points"][:n], s["materials"][:n], capi.DL_ALL)
            assert_table(got, s, n, slice(0, n))
            ds.occluded(t["rays"][:max(1, n // 3)], t["dist"][:max(1, n // 3)])
            m = min(n, len(s["rays"]))
            r = ds.direct_light_rays(s["rays"][:m], capi.DL_RADIANCE | capi.DL_DIFFUSE)
            keep = s["index"][s["index"] < m]
            assert_same(r["diffuse"][keep], s["diffuse"][:len(keep)], (n, "rays"))
            ds.light_transmittance(s["points"][:max(1, n // 2), :6])
            shared = ds.direct_light(s["points"][:n], s["materials"][0], capi.DL_DIFFUSE)
            assert_same(shared["diffuse"], got["diffuse"], (n, "shared"))   # no material in diffuse
            ds.intersect_rays(s["rays"][:max(1, m // 2)])
        ds.close()


# ------------------------------------------------------------------ device tensors, streams
def test_device_entries_on_a_caller_stream(oracle):
    """On a stream set through rt_context_set_stream the answers are there once that stream has
    synchronised."""
    s = dl.scene_set("glass")
    with capi.Context(0) as c:
        ds = c.scene(s["sc"])
        stream = torch.cuda.Stream()
        c.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            d_pts = torch.from_numpy(s["points"].copy()).to("cuda", non_blocking=False)
            d_mat = torch.from_numpy(s["materials"].copy()).to("cuda", non_blocking=False)
            d_rays = torch.from_numpy(s["rays"].copy()).to("cuda", non_blocking=False)
            a = ds.direct_light_device(d_pts, d_mat, capi.DL_ALL)
            b = ds.direct_light_rays_device(d_rays, capi.DL_ALL)
        stream.synchronize()
        got = {k: v.cpu().numpy() for k, v in a.items()}
        assert all(v.dtype == np.float64 and v.shape == (len(s["points"]), 3) for v in got.values())
        assert_table(got, s, "glass stream")
        rays = {k: v.cpu().numpy()[s["index"]] for k, v in b.items()}
        assert_table(rays, s, "glass rays stream", slice(0, s["n_hits"]))
        c.set_stream(None)
        ds.close()


# ------------------------------------------------------------------ no lights, empty scene
def test_scene_without_lights_and_empty_scene(ctx, oracle):
    """A scene without lights writes zeros for the requested outputs (their shape is fixed), for
    hits and misses alike; so does an empty scene, where every ray misses."""
    s = dl.scene_set("c2")
    dark = SceneData(s["sc"].camera, s["sc"].spheres, s["sc"].planes)
    for sc in (dark, SceneData(s["sc"].camera)):
        ds = ctx.scene(sc)
        try:
            n = len(s["rays"])
            d_rays = torch.from_numpy(s["rays"].copy()).cuda()
            d_pts = torch.from_numpy(s["points"].copy()).cuda()
            out_r = {k: torch.full((n, 3), FILL, dtype=torch.float64, device="cuda") for k in NAMES}
            out_p = {k: torch.full((len(s["points"]), 3), FILL, dtype=torch.float64, device="cuda")
                     for k in NAMES}
            torch.cuda.synchronize()
            ds.direct_light_rays_device(d_rays, capi.DL_ALL, out=out_r)
            ds.direct_light_device(d_pts, tuple(s["materials"][0]), capi.DL_ALL, out=out_p)
            ctx.synchronize()
            host_r = ds.direct_light_rays(s["rays"], capi.DL_ALL)
            host_p = ds.direct_light(s["points"], s["materials"], capi.DL_ALL)
            for k in NAMES:
                for v in (out_r[k].cpu().numpy(), out_p[k].cpu().numpy(), host_r[k], host_p[k]):
                    assert v.shape[1] == 3 and not bits(v).any(), k
            assert ds.direct_light_rays(np.empty((0, 6)), capi.DL_ALL)["diffuse"].shape == (0, 3)
            assert ds.direct_light(np.empty((0, 9)), s["materials"][0])["radiance"].shape == (0, 3)
        finally:
            ds.close()


# ------------------------------------------------------------------ non-finite inputs
@pytest.mark.parametrize("name", ["c2", "c3", "glass", "mesh"])
def test_nonfinite_points(ctx, oracle, name):
    """Zero, NaN, infinite, 2^±500 and denormal components in p, normal and view: the call
    returns (the march is bounded by its 64 steps, the BVH stack by its 64 entries) and follows
    IEEE through the same expressions as the restatement: diffuse has its bits, NaNs where it
    has NaNs."""
    sc, pts, mats = dl.nonfinite_points(name)
    e = dl.expected(sc, pts, mats)
    ds = ctx.scene(sc)
    try:
        got = ds.direct_light(pts, mats, capi.DL_ALL)
        bad = np.flatnonzero((dl.canonical_bits(got["diffuse"]) != dl.canonical_bits(e["diffuse"])).any(axis=1))
        assert not len(bad), (name, len(bad), pts[bad[:4]], got["diffuse"][bad[:4]], e["diffuse"][bad[:4]])
        for k in ("specular", "radiance"):
            assert np.array_equal(np.isnan(got[k]), np.isnan(e[k])), (name, k)
            ok = dl.within_bar(got[k], e[k]) | np.isnan(e[k]) | (got[k] == e[k])
            assert ok.all(), (name, k, np.argwhere(~ok)[:4])
        # (the reference's guards — max(0, NaN) is 0, a NaN length skips the light — keep NaN out
        # of these tables; the special values that leave a light on are the ones that matter)
        assert ((np.nan_to_num(e["diffuse"]) != 0.0).any(axis=1)).sum() >= 20
        assert_composed(got, mats, name)
    finally:
        ds.close()


@pytest.mark.parametrize("name", ts.NONFINITE_SCENES)
def test_nonfinite_rays(ctx, oracle, name):
    """Zero, NaN, infinite, huge and denormal o and d: the call returns, and where the oracle's
    IntersectClosest reports a hit the diffuse is the restatement's on that hit."""
    sc = raysets.scene(name)
    rays = raysets.nonfinite_rays(sc)
    h = dl.hits(sc, rays, finite_only=False)
    e = dl.expected(sc, h["points"], h["materials"])
    ds = ctx.scene(sc)
    try:
        got = ds.direct_light_rays(rays, capi.DL_ALL)
        assert got["diffuse"].shape == (len(rays), 3)
        miss = np.setdiff1d(np.arange(len(rays)), h["index"])
        assert not bits(got["diffuse"][miss]).any() and not bits(got["radiance"][miss]).any()
        d = got["diffuse"][h["index"]]
        bad = np.flatnonzero((dl.canonical_bits(d) != dl.canonical_bits(e["diffuse"])).any(axis=1))
        assert not len(bad), (name, len(bad), rays[h["index"]][bad[:4]], d[bad[:4]], e["diffuse"][bad[:4]])
    finally:
        ds.close()


# ------------------------------------------------------------------ C++ drop-in API
@pytest.mark.parametrize("name", ["c2", "glass"])
def test_cpp_batches_equal_single_point_host(oracle, tmp_path, name):
    """examples/direct_light_scenefile: Scene::DirectLightning(rays) and
    Scene::DirectLightning(hits, viewDirs, normals) on the GPU and the single-point host method
    agree with each other and with the table: bit for bit without pow, within the bar with it."""
    s = dl.scene_set(name)
    scene = tmp_path / "scene.txt"
    s["sc"].write(scene)
    s["rays"].tofile(tmp_path / "rays.f64")
    subprocess.run([EXE, str(scene), str(tmp_path / "rays.f64"), str(tmp_path)], check=True,
                   capture_output=True, timeout=120)
    want = np.zeros((s["n_rays"], 3), np.float64)
    want[s["index"]] = s["radiance"][:s["n_hits"]]
    exact = np.ones(s["n_rays"], bool)
    exact[s["index"]] = ~s["pow"][:s["n_hits"]]
    res = {k: np.fromfile(tmp_path / f"{k}.f64", np.float64).reshape(-1, 3)
           for k in ("batch_rays", "batch_points", "single")}
    assert_same(res["batch_rays"], res["batch_points"], (name, "the two batches"))
    for k, v in res.items():
        assert_same(v[exact], want[exact], (name, k))
        assert dl.within_bar(v, want).all(), (name, k)
        assert dl.within_bar(v, res["single"]).all(), (name, k, "against the host method")
    assert (want != 0.0).any() and (name == "c2" or not exact.all())
