"""rt_occluded_rays / rt_occluded_rays_device (occluded_rays_kernel, rt_anyhit.hip): the batch
Scene::IntersectAnyBefore (Scene.h:259-276) on the ray sets of tests/raysets.py.

The comparator is the table of tests/occlusion_sets.py: per ray the smallest positive t of the
oracle's per-shape Intersect functions, the answer for a maxDist being `tpos < maxDist`.  Every
ray is asked with distances one unit in the last place around its tpos, so the bar is the bits of
t and the strict '<': byte equality everywhere, no tolerance.  That the tables ask on both sides
is asserted on the CPU in tests/test_oracle_occlusion.py."""
import os
import subprocess

import numpy as np
import pytest
import torch

import occlusion_sets as oc
import raysets
from raytracingengine_amd import capi
from raytracingengine_amd.scene import SceneData

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "bin", "occlusion_scenefile")
SIZES = (0, 1, 63, 64, 65, 255, 256, 257)
GUARD = 64


def assert_table(got, t, what):
    assert got.dtype == np.bool_ and got.shape == t["expected"].shape
    raw = got.view(np.uint8)
    assert ((raw == 0) | (raw == 1)).all(), what
    bad = np.flatnonzero(got != t["expected"])
    assert not len(bad), (what, len(bad), bad[:8], t["rays"][bad[:4]], t["dist"][bad[:4]],
                          t["tpos"][t["index"][bad[:4]]])


def run_table(ctx, t, what):
    ds = ctx.scene(t["sc"])
    try:
        assert_table(ds.occluded(t["rays"], t["dist"]), t, what)
    finally:
        ds.close()


@pytest.fixture(scope="module")
def c2(ctx, oracle):
    t = oc.scene_table("c2")
    ds = ctx.scene(t["sc"])
    yield ds, t
    ds.close()


# ------------------------------------------------------------------ values
@pytest.mark.parametrize("name", list(raysets.SCENES))
def test_scenes(ctx, oracle, name):
    run_table(ctx, oc.scene_table(name), name)


@pytest.mark.parametrize("name", list(raysets.CRAFTED))
def test_crafted_sets(ctx, oracle, name):
    run_table(ctx, oc.crafted_table(name), name)


@pytest.mark.parametrize("name", oc.NONFINITE_SCENES)
def test_nonfinite_rays(ctx, oracle, name):
    """Zero, NaN, infinite, huge and denormal rays: the call returns (every loop is bounded by
    the scene's size) and follows IEEE through the same expressions as the oracle."""
    run_table(ctx, oc.nonfinite_table(name), f"{name} nonfinite")


def test_plane_at_zero(ctx, oracle):
    """Origins on a plane: the plane's t == 0 does not count and does not hide the sphere
    further along, which a closest hit compared with maxDist would miss."""
    sc, rays = oc.plane_at_zero()
    tp = oc.tpos(sc, rays)
    ds = ctx.scene(sc)
    try:
        for max_dist in (10.0, np.inf, 4.0, raysets.step(4.0, 1)):
            got = ds.occluded(rays, max_dist)
            assert np.array_equal(got, tp < max_dist), max_dist
        assert list(ds.occluded(rays, 10.0)) == [True, True, False, False]
        cl = ds.intersect_rays(rays)
        assert (cl[:, 0] == 2).all() and (cl[:, 2] == 0.0).all()   # what the other route sees
    finally:
        ds.close()


# ------------------------------------------------------------------ BVH
@pytest.mark.parametrize("name", oc.BVH_SCENES + oc.BVH_GRIDS)
def test_bvh_equals_every_triangle(ctx, oracle, name):
    """The any-hit traversal gives the bytes of the plain loop over all triangles
    (RT_FLAG_NO_BVH) — on bigmesh for its whole ray set, with each ray's distances taken from the
    device's own closest hit where the table stops."""
    if name in oc.BVH_GRIDS:
        t = oc.crafted_table(name)
        sc, rays, dist = t["sc"], t["rays"], t["dist"]
    else:
        sc = raysets.scene(name)
        base, _ = raysets.rayset(sc)
    ds = ctx.scene(sc)
    try:
        if name in oc.BVH_SCENES:
            cl = ds.intersect_rays(base)
            tp = np.where((cl[:, 0] != 0) & (cl[:, 2] > 0.0), cl[:, 2], np.inf)
            rays, dist, _, _ = oc.pairs(base, tp)
        assert len(sc.triangle_array()) >= 32       # a BVH is built
        with_bvh = ds.occluded(rays, dist)
        without = ds.occluded(rays, dist, no_bvh=True)
        assert np.array_equal(with_bvh.view(np.uint8), without.view(np.uint8))
        assert 0.2 <= with_bvh.mean() <= 0.8
    finally:
        ds.close()


# ------------------------------------------------------------------ sizes, guards, repeats
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_guard_bytes(ctx, c2, n):
    """n around the wave and workgroup sizes: the host entry gives the table's first n answers;
    the device entry writes n bytes of 0 / 1 and leaves the 64 bytes after them alone; a second
    call gives the same bytes."""
    ds, t = c2
    rays, dist, want = t["rays"][:n], t["dist"][:n], t["expected"][:n]
    got = ds.occluded(rays, dist)
    assert got.shape == (n,) and np.array_equal(got, want)
    assert np.array_equal(ds.occluded(rays, dist), got)
    d_rays = torch.from_numpy(rays.copy()).cuda()
    d_dist = torch.from_numpy(dist.copy()).cuda()
    out = torch.full((n + GUARD,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for _ in range(2):
        assert ds.occluded_device(d_rays, d_dist, out=out) is out
        ctx.synchronize()
        h = out.cpu().numpy()
        assert (h[n:] == 0xCD).all()
        assert np.array_equal(h[:n], want.astype(np.uint8))


def test_buffer_grows_and_shrinks(oracle):
    """ctx->rays (7 doubles and a byte per ray here) grows on demand: growing and shrinking n on
    one fresh context, with the other batch entries in between, gives the table each time."""
    t = oc.scene_table("mesh")
    with capi.Context(0) as c:
        ds = c.scene(t["sc"])
        for n in (3, 1000, 64, len(t["dist"]), 1, 257):
            got = ds.occluded(t["rays"][:n], t["dist"][:n])
            assert np.array_equal(got, t["expected"][:n]), n
            ds.intersect_rays(t["rays"][:max(1, n // 2)])
        ds.close()


# ------------------------------------------------------------------ device tensors
def test_device_tensors_equal_host_entry(ctx, oracle):
    t = oc.scene_table("mesh")
    ds = ctx.scene(t["sc"])
    try:
        host = ds.occluded(t["rays"], t["dist"])
        d_rays = torch.from_numpy(t["rays"].copy()).cuda()
        d_dist = torch.from_numpy(t["dist"].copy()).cuda()
        torch.cuda.synchronize()
        out = ds.occluded_device(d_rays, d_dist)
        ctx.synchronize()
        assert out.dtype == torch.uint8 and out.shape == (len(host),)
        assert np.array_equal(out.cpu().numpy(), host.view(np.uint8))
        out = ds.occluded_device(d_rays, d_dist, no_bvh=True)
        ctx.synchronize()
        assert np.array_equal(out.cpu().numpy(), host.view(np.uint8))
        assert_table(host, t, "mesh")
    finally:
        ds.close()


def test_device_entry_on_a_caller_stream(oracle):
    """On a stream set through rt_context_set_stream the answers are there once that stream has
    synchronised."""
    t = oc.scene_table("c2")
    with capi.Context(0) as c:
        ds = c.scene(t["sc"])
        stream = torch.cuda.Stream()
        c.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            d_rays = torch.from_numpy(t["rays"].copy()).to("cuda", non_blocking=False)
            d_dist = torch.from_numpy(t["dist"].copy()).to("cuda", non_blocking=False)
            out = torch.full((len(t["dist"]),), 0xCD, dtype=torch.uint8, device="cuda")
            ds.occluded_device(d_rays, d_dist, out=out)
        stream.synchronize()
        assert np.array_equal(out.cpu().numpy(), t["expected"].astype(np.uint8))
        c.set_stream(None)
        ds.close()


# ------------------------------------------------------------------ scalar maxDist, empty scene
def test_scalar_max_dist_and_empty_scene(ctx, c2):
    ds, t = c2
    base, tp = t["base"], t["tpos"]
    d_rays = torch.from_numpy(base.copy()).cuda()
    torch.cuda.synchronize()
    finite = np.sort(tp[np.isfinite(tp)])
    for max_dist in (float(finite[len(finite) // 2]), np.inf, 0.0, np.nan):
        with np.errstate(invalid="ignore"):
            want = tp < max_dist
        assert np.array_equal(ds.occluded(base, max_dist), want), max_dist
        out = ds.occluded_device(d_rays, max_dist)
        ctx.synchronize()
        assert np.array_equal(out.cpu().numpy(), want.astype(np.uint8)), max_dist
    assert 0.2 <= (tp < float(finite[len(finite) // 2])).mean() <= 0.8
    empty = ctx.scene(SceneData(t["sc"].camera))
    try:
        assert not empty.occluded(base, np.inf).any()
        assert not empty.occluded(t["rays"], t["dist"]).any()
        assert empty.occluded(np.empty((0, 6)), 1.0).shape == (0,)
    finally:
        empty.close()


# ------------------------------------------------------------------ C++ drop-in API
@pytest.mark.parametrize("name", ["c2", "mesh"])
def test_cpp_batch_equals_single_ray_host(oracle, tmp_path, name):
    """examples/occlusion_scenefile: Scene::IntersectAnyBefore(rays, maxDist) on the GPU and the
    single-ray host method give the same bytes, and both are the table."""
    t = oc.scene_table(name)
    scene = tmp_path / "scene.txt"
    t["sc"].write(scene)
    t["rays"].tofile(tmp_path / "rays.f64")
    t["dist"].tofile(tmp_path / "dist.f64")
    subprocess.run([EXE, str(scene), str(tmp_path / "rays.f64"), str(tmp_path / "dist.f64"),
                    str(tmp_path)], check=True, capture_output=True, timeout=120)
    batch = np.fromfile(tmp_path / "batch.u8", np.uint8)
    single = np.fromfile(tmp_path / "single.u8", np.uint8)
    assert np.array_equal(batch, single)
    assert np.array_equal(batch, t["expected"].astype(np.uint8))
