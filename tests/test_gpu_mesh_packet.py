"""The packet kernels' triangle path on the crafted mesh scenes of tests/mesh_sets.py: the
wave-coherent BVH walk (bvh_wave, csrc/rt_packet_device.hpp) for the camera rays and the exact
shadow march of packet_direct_kernel's kFeatTris and kFeatAll variants, and for the packet
G-buffer kernel (rt_gbuffer.hip, TRIS).

Reference: the C oracle alone — oracle.render for the frames and their ray counts, and
oracle.closest_rays on the oracle's own camera rays for the G-buffer.  Every comparison is on the
bits, except the frames with Blinn-Phong switched on (libm pow: POW_TOL) and the Reinhard-Jodie
bytes (tonemap_sets.check_bytes, as tests/test_gpu_tonemap.py).  The same frame is asked of the
counting, the single-sample and the multi-sample instantiation, of the packet kernel's plain
triangle loop (RT_FLAG_NO_BVH) and of the per-lane walk (RT_FLAG_GENERIC_KERNEL), so a mismatch
names its side.  tests/test_mesh_sets.py holds, on the CPU, that the scenes have the edges they
exist for; tests/test_bvh_walk_host.py holds that the depth-cap tree of the fan scenes fits every
walk's stack, and is to pass before those scenes meet a GPU.
"""
import numpy as np
import pytest

import mesh_sets as ms
import tonemap_sets as tm
from direct_light_sets import POW_TOL
from raytracingengine_amd import capi
from test_gpu_gbuffer import _expected, _frame_rows, _same
from test_gpu_packet_uniform import _batch

pytestmark = pytest.mark.gpu

NO_BVH, GENERIC = capi.RT_FLAG_NO_BVH, capi.RT_FLAG_GENERIC_KERNEL
BATCH_CAMERAS = [(0.0, 0.0, -2.0), (1.0, 0.0, -2.0), (0.0, 1.0, -3.0)]
ROW_SETS = [dict(row_begin=3, row_end=29), dict(row_begin=8, row_block=8, row_cycle=3)]


@pytest.fixture(scope="module")
def cases(ctx, oracle):
    """Per scene: the uploaded scene, its data, and what the oracle says of it (mesh_sets.facts:
    the frame, its ray counts, the camera rays and their closest hits), computed once."""
    out = {}
    for name, make in ms.SCENES.items():
        sc = make()
        out[name] = (ctx.scene(sc), sc, ms.facts(sc))
    yield out
    for ds, _, _ in out.values():
        ds.close()


def _gb_reference(sc, f):
    return _expected(sc, f["closest"], sc.camera.height)


# ------------------------------------------------------------------ render, per scene
@pytest.mark.parametrize("name", list(ms.SCENES))
def test_render_is_the_oracles_frame(ctx, cases, name):
    ds, sc, f = cases[name]
    ref = f["image"]
    out = ds.render(hdr64=True, tonemap=1, stats=True)                 # COUNT
    assert tm.same(out["hdr64"], ref), "counting"
    assert (out["trace_rays"], out["shadow_rays"]) == (f["trace_rays"], f["shadow_rays"])
    assert np.array_equal(out["ldr"], tm.po.tonemap(ref, 1).reshape(ref.shape))
    # rt_debug_cone_table counts the packet kernel's frames (with, without) a cone table: the
    # default render is one (a triangle variant reads no table), the generic render is none
    before = ctx.debug_cone_table()
    assert tm.same(ds.render(hdr64=True, tonemap=1)["hdr64"], ref), "single sample"
    packet = ctx.debug_cone_table()
    assert tm.same(ds.render(hdr64=True, tonemap=1, flags=NO_BVH)["hdr64"], ref), "triangle loop"
    mid = ctx.debug_cone_table()
    assert tm.same(ds.render(hdr64=True, tonemap=1, flags=GENERIC)["hdr64"], ref), "per-lane walk"
    after = ctx.debug_cone_table()
    assert (packet[0] - before[0], packet[1] - before[1]) == (0, 1), "not the packet kernel"
    assert (mid[0] - packet[0], mid[1] - packet[1]) == (0, 1), "not the packet kernel"
    assert after == mid, "the generic render took the packet kernel"
    jodie = ds.render(hdr64=True, tonemap=tm.JODIE)                    # kFeatAll through kFeatJodie
    assert tm.same(jodie["hdr64"], ref), "kFeatAll"
    worst = tm.assert_bytes(jodie["ldr"], ref, tm.JODIE, f"{name} operator 4")
    print(f"{name}: largest operator-4 distance {worst:.3g} ulps")


# ------------------------------------------------------------------ variants
@pytest.fixture(scope="module")
def variant_scene(ctx):
    made = []

    def make(sc):
        made.append(ctx.scene(sc))
        return made[-1]
    yield make
    for ds in made:
        ds.close()


@pytest.mark.parametrize("name", ms.VARIANT_SCENES)
def test_four_samples(variant_scene, oracle, name):
    """aa = 4, the MULTI instantiation (counting and not)."""
    sc = ms.with_aa(ms.SCENES[name](), 4)
    ref, nt, ns = oracle.render(sc, seed=1234)
    ds = variant_scene(sc)
    out = ds.render(hdr64=True, stats=True, seed=1234)
    assert tm.same(out["hdr64"], ref)
    assert (out["trace_rays"], out["shadow_rays"]) == (nt, ns)
    assert tm.same(ds.render(hdr64=True, seed=1234)["hdr64"], ref)


def _most_seen_triangle(sc):
    f = ms.facts(sc)
    return int(np.bincount(f["lowest"][f["hit"]]).argmax())


@pytest.mark.parametrize("name", ms.VARIANT_SCENES)
def test_blinn_phong_switched_on(variant_scene, oracle, name):
    """One triangle with specular 5e-4 (not above the bias: still the direct path; above 0:
    kFeatAll with the Blinn-Phong term).  pow is libm's in the oracle: POW_TOL; the BVH and the
    plain loop run the same shading, so they agree on the bits."""
    base = ms.SCENES[name]()
    sc = ms.with_specular(base, _most_seen_triangle(base))
    ref, _, _ = oracle.render(sc)
    assert not tm.same(ref, oracle.render(base)[0])          # the term is in the image
    ds = variant_scene(sc)
    got = ds.render(hdr64=True)["hdr64"]
    d = np.abs(got - ref).max()
    print(f"{name}: Blinn-Phong frame max |d| {d:.3g}")
    assert d <= POW_TOL
    assert tm.same(ds.render(hdr64=True, flags=NO_BVH)["hdr64"], got)


@pytest.mark.parametrize("kw", ROW_SETS)
@pytest.mark.parametrize("name", ms.VARIANT_SCENES)
def test_row_sets_off_the_tile_edges(cases, name, kw):
    ds, sc, f = cases[name]
    o = capi.default_opts(**kw)
    rows = _frame_rows(o, sc.camera.height)
    assert 0 < len(rows) == capi.rendered_rows(o, sc.camera.height) < sc.camera.height
    assert tm.same(ds.render(hdr64=True, **kw)["hdr64"], f["image"][rows])


@pytest.mark.parametrize("name", ms.VARIANT_SCENES)
def test_batch_of_three_cameras(ctx, cases, oracle, name):
    ds, sc, _ = cases[name]
    frames = _batch(ctx, ds, sc, BATCH_CAMERAS, capi.default_opts(tonemap=1))
    for pos, (hdr, ldr) in zip(BATCH_CAMERAS, frames):
        ref, _, _ = oracle.render(ms.moved(sc, pos))
        assert tm.same(hdr, ref), pos
        assert np.array_equal(ldr, tm.po.tonemap(ref, 1).reshape(ldr.shape)), pos
    assert not tm.same(frames[0][0], frames[1][0])


# ------------------------------------------------------------------ G-buffer, per scene
@pytest.mark.parametrize("name", list(ms.SCENES))
def test_gbuffer_is_the_oracles_closest_hit(ctx, cases, monkeypatch, name):
    ds, sc, f = cases[name]
    ref = _gb_reference(sc, f)
    _same(ds.gbuffer(), ref, "packet")
    monkeypatch.setenv("RTAMD_GB_TILE", "16")
    _same(ds.gbuffer(), ref, "packet, 16x4 tiles")
    monkeypatch.delenv("RTAMD_GB_TILE")
    _same(ds.gbuffer(opts=capi.default_opts(flags=NO_BVH)), ref, "triangle loop")
    hits = ds.closest_device(ds.camera_rays_device(0),
                             outputs=capi.CH_T | capi.CH_PRIM | capi.CH_NORMAL)
    ctx.synchronize()
    shape = ref["depth"].shape
    got = {"depth": hits["t"].cpu().numpy().reshape(shape),
           "prim": hits["prim"].cpu().numpy().reshape(*shape, 2),
           "normal": hits["normal"].cpu().numpy().reshape(*shape, 3)}
    _same(got, {k: ref[k] for k in got}, "closest_device of camera_rays_device")


@pytest.mark.parametrize("name", ["wall", "fan"])
def test_ties_go_to_the_lowest_index(cases, name):
    """Every camera ray on which two or more triangles accept with the same smallest t (counted
    by tests/test_mesh_sets.py) names the lowest index among them."""
    ds, sc, f = cases[name]
    prim = ds.gbuffer(outputs=capi.GB_PRIM)["prim"].reshape(-1, 2)
    ties = f["ties"]
    assert ties.sum() >= 500
    assert np.all(prim[ties, 0] == 3)
    assert np.array_equal(prim[ties, 1], f["lowest"][ties].astype(np.int32))
