"""The full-frame G-buffer pass on the GPU (rt_gbuffer / rt_gbuffer_device, rt_gbuffer.hip).

Reference: rt_intersect_rays (pinned to the oracle and to the compiled reference on arbitrary
rays — sphere, triangle and BVH edge cases, origins inside and on surfaces, any direction
length — by test_gpu_ray_queries.py, and on camera-like rays by the known-answer tests of
test_gpu_parity.py) fed with the oracle's Camera::getRay of every pixel; every 7th pixel is also
checked against the oracle's own IntersectClosest.  Every comparison is on the bits
(np.array_equal); depth_norm and albedo against numpy's float32 rounding of the reference doubles.
"""
import ctypes
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from raytracingengine_amd import capi
from raytracingengine_amd.configs import (_random_sphere_scene, glass_scene, make_config,
                                          mesh_scene, mirror_scene, reference_box)
from raytracingengine_amd.scene import Camera, Material, SceneData

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "bin", "gbuffer_scenefile")
NAMES = [n for n, _, _, _ in capi.GB_OUTPUTS]


def _bare(width, height):
    return SceneData(Camera((0.0, 0.0, -25.0), width / 2.0, width, height, 0.0, 200.0, 1))


def _coincident():
    sc = _bare(48, 32)
    sc.add_sphere((0.0, 0.0, 5.0), 4.0, Material((1.0, 0.0, 0.0)))
    sc.add_sphere((0.0, 0.0, 5.0), 4.0, Material((0.0, 1.0, 0.0)))
    return sc


def _inside():
    sc = _bare(48, 32)
    sc.add_sphere((1.0, -2.0, -24.0), 30.0, Material((0.2, 0.4, 0.8)))  # holds the camera
    sc.add_sphere((0.0, 0.0, 60.0), 5.0, Material((1.0, 1.0, 1.0)))     # outside it: hidden
    return sc


SCENES = {
    "c2_37x21": lambda: make_config("c2", 37, 21),
    "c2_1x1": lambda: make_config("c2", 1, 1),
    "c2_5x64": lambda: make_config("c2", 5, 64),
    "spheres70": lambda: _random_sphere_scene("c3", 61, 35, 70, 2, 1, 1),
    "spheres300": lambda: _random_sphere_scene("c4", 61, 35, 300, 1, 1, 1),
    "coincident": _coincident,
    "inside": _inside,
    "empty": lambda: _bare(33, 17),
    "box": lambda: reference_box().resized(40, 40),
    "mirror": lambda: mirror_scene(56, 32),
    "glass": lambda: glass_scene(56, 32),
    "mesh": lambda: mesh_scene(96, 64),
}
# every scene above is inside the packet kernel's limits (<= 1024 spheres, image <= 40 KiB)


def _frame_rows(o, height):
    """Image rows of the rows-local output, in order (rt_render_opts)."""
    r1 = min(o.row_end, height) if o.row_end else height
    if o.row_cycle <= 1 or o.row_block == 0:
        return list(range(o.row_begin, r1))
    rows = []
    for b in range(o.row_begin, r1, o.row_block * o.row_cycle):
        rows += list(range(b, min(b + o.row_block, r1)))
    return rows


def _reference(ds, sc, oracle, rows, near=None, far=None):
    """The expected outputs for image rows `rows` of sc's camera, from rt_intersect_rays."""
    cam = sc.camera
    W = cam.width
    L, osc = oracle.lib(), oracle.OracleScene(sc)  # pyoracle.get_ray / closest, one scene view
    rays = np.empty((len(rows) * W, 6), np.float64)
    for j, y in enumerate(rows):
        for x in range(W):
            L.oracle_get_ray(osc.camera.ctypes.data, x, y, 0, 0, 0, rays[j * W + x].ctypes.data)
    hits = ds.intersect_rays(rays)
    o7, index = np.zeros(7, np.float64), ctypes.c_int32(-1)
    for i in range(0, len(rays), 7):  # the reference's own IntersectClosest
        typ = L.oracle_closest(ctypes.addressof(osc.c), rays[i].ctypes.data, o7.ctypes.data,
                               ctypes.byref(index))
        idx = index.value if typ else -1
        assert (typ, idx) == (int(hits[i, 0]), int(hits[i, 1])), i
        if typ:
            assert np.array_equal(o7[:4], hits[i, 2:6]), i  # distance, normal
    return _expected(sc, hits, len(rows), near, far)


def _expected(sc, hits, n, near=None, far=None):
    """The pass's outputs for n image rows from their rays' closest hits ([n * W, 9] in
    rt_intersect_rays' layout, the oracle's closest_rays included)."""
    cam = sc.camera
    W = cam.width
    hit = hits[:, 0] != 0
    mats = np.concatenate([a["material"]["color"].reshape(-1, 3) for a in
                           (sc.sphere_array(), sc.plane_array(), sc.triangle_array())] +
                          [np.zeros((1, 3))])
    base = np.array([0, 0, len(sc.spheres), len(sc.spheres) + len(sc.planes)])
    slot = np.where(hit, base[hits[:, 0].astype(int)] + hits[:, 1].astype(int), len(mats) - 1)
    t = np.where(hit, hits[:, 2], np.inf)
    near = cam.near_plane if near is None else near
    far = cam.far_plane if far is None else far
    with np.errstate(all="ignore"):
        dn = ((t - near) / (far - near)).astype(np.float32)
    return {
        "depth": t.reshape(n, W),
        "depth_norm": np.where(hit, dn, np.float32(np.inf)).astype(np.float32).reshape(n, W),
        "normal": np.where(hit[:, None], hits[:, 3:6], 0.0).reshape(n, W, 3),
        "prim": hits[:, :2].astype(np.int32).reshape(n, W, 2),
        "albedo": mats[slot].astype(np.float32).reshape(n, W, 3),
    }


def _same(got, ref, what=""):
    assert sorted(got) == sorted(ref), what
    for k in ref:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k)
        # bits, not values: -0.0 and NaN payloads count
        assert np.array_equal(got[k].view(np.uint8), ref[k].view(np.uint8)), (what, k)


@pytest.fixture(scope="module")
def cases(ctx, oracle):
    """Per scene: the uploaded scene, its data and the full-frame reference, computed once."""
    out = {}
    for name, make in SCENES.items():
        sc = make()
        ds = ctx.scene(sc)
        out[name] = (ds, sc, _reference(ds, sc, oracle, range(sc.camera.height)))
    yield out
    for ds, _, _ in out.values():
        ds.close()


@pytest.mark.parametrize("name", list(SCENES))
def test_packet_and_generic_match_intersect_rays(cases, name):
    ds, sc, ref = cases[name]
    got = ds.gbuffer()
    _same(got, ref, "packet")
    _same(ds.gbuffer(opts=capi.default_opts(flags=capi.RT_FLAG_GENERIC_KERNEL)), ref, "generic")
    if name == "empty":  # the exact miss encoding
        assert np.all(got["prim"] == np.array([0, -1], np.int32))
        assert np.all(np.isposinf(got["depth"])) and np.all(np.isposinf(got["depth_norm"]))
        assert not got["normal"].view(np.uint8).any() and not got["albedo"].view(np.uint8).any()
    if name == "coincident":  # the lowest index wins a tie
        assert set(np.unique(got["prim"][..., 1])) == {-1, 0}
    if name == "inside":  # the far root of the sphere around the camera, everywhere
        assert np.all(got["prim"] == np.array([1, 0], np.int32))
    if name.startswith("spheres"):  # scene indices, not chunk-order ones: checked by albedo too
        assert got["prim"][..., 1].max() >= 64


def test_both_tile_shapes(cases, monkeypatch):
    """The packet kernel's 8x8 and 16x4 tiles (RTAMD_GB_TILE) give the same frame."""
    for name in ("c2_37x21", "spheres300", "mesh"):
        ds, _, ref = cases[name]
        for tile in ("8", "16"):
            monkeypatch.setenv("RTAMD_GB_TILE", tile)
            _same(ds.gbuffer(), ref, f"{name} tile {tile}")


@pytest.mark.parametrize("kw", [dict(row_begin=3, row_end=18),
                                dict(row_begin=8, row_block=8, row_cycle=3)])
@pytest.mark.parametrize("flags", [0, capi.RT_FLAG_GENERIC_KERNEL])
def test_row_sets(ctx, oracle, kw, flags):
    """A contiguous range off any tile edge, and block-cyclic rows (rank 1 of 3)."""
    sc = make_config("c2", 37, 21) if "row_end" in kw else make_config("c2", 40, 64)
    ds = ctx.scene(sc)
    o = capi.default_opts(flags=flags, **kw)
    rows = _frame_rows(o, sc.camera.height)
    assert len(rows) == capi.rendered_rows(o, sc.camera.height) and len(rows) < sc.camera.height
    _same(ds.gbuffer(opts=o), _reference(ds, sc, oracle, rows))
    ds.close()


def test_mesh_without_bvh(cases):
    ds, _, ref = cases["mesh"]
    assert (ref["prim"][..., 0] == 3).any()
    for flags in (capi.RT_FLAG_NO_BVH, capi.RT_FLAG_NO_BVH | capi.RT_FLAG_GENERIC_KERNEL):
        _same(ds.gbuffer(opts=capi.default_opts(flags=flags)), ref, flags)


@pytest.mark.parametrize("name", ["c2_37x21", "mesh"])
def test_each_output_alone(cases, name):
    ds, _, ref = cases[name]
    for out_name, bit, _, _ in capi.GB_OUTPUTS:
        _same(ds.gbuffer(outputs=bit), {out_name: ref[out_name]}, out_name)
    two = capi.GB_DEPTH | capi.GB_PRIM
    _same(ds.gbuffer(outputs=two), {"depth": ref["depth"], "prim": ref["prim"]})


@pytest.mark.parametrize("flags", [0, capi.RT_FLAG_GENERIC_KERNEL])
def test_batch_equals_single_frames(ctx, oracle, flags):
    sc = make_config("c2", 37, 21)
    ds = ctx.scene(sc)
    pos = [(0.0, 0.0, -25.0), (3.0, 1.0, -22.0), (-4.0, -2.0, -30.0)]
    o = capi.default_opts(flags=flags)
    got = ds.gbuffer(cams=ds.cameras(pos), opts=o)
    for f, p in enumerate(pos):
        moved = dataclasses.replace(sc, camera=dataclasses.replace(sc.camera, position=p))
        one = ctx.scene(moved)
        single = one.gbuffer(opts=o)
        _same({k: v[f] for k, v in got.items()}, single, f)
        if f == 1:
            _same(single, _reference(one, moved, oracle, range(21)))
        one.close()
    ds.close()


def test_host_entry_equals_device_entry(cases):
    ds, sc, ref = cases["spheres70"]
    dev = ds.gbuffer(cams=ds.cameras([sc.camera.position]))
    _same({k: v[0] for k, v in dev.items()}, ref)


def test_near_far_change_depth_norm_only(ctx, cases, oracle):
    _, sc, ref = cases["c2_37x21"]
    moved = dataclasses.replace(sc, camera=dataclasses.replace(sc.camera, near_plane=0.5,
                                                               far_plane=80.0))
    ds = ctx.scene(moved)
    got = ds.gbuffer()
    want = _reference(ds, moved, oracle, range(21))
    _same(got, want)
    for k in NAMES:
        assert np.array_equal(got[k], ref[k]) == (k != "depth_norm"), k
    ds.close()


def test_opts_fields_that_are_not_read(cases):
    """max_recursion, bias, seed and tonemap do not steer the pass (nor fail it)."""
    ds, _, ref = cases["mirror"]
    o = capi.default_opts(max_recursion=64, bias=0.5, seed=7, tonemap=99)
    _same(ds.gbuffer(opts=o), ref)


def test_cpp_example_matches_binding(cases, tmp_path):
    ds, sc, ref = cases["c2_37x21"]
    scene = tmp_path / "scene.txt"
    sc.write(scene)
    subprocess.run([EXE, str(scene), str(tmp_path)], check=True, capture_output=True, timeout=120)
    files = {"depth": "depth.f64", "depth_norm": "depth_norm.f32", "normal": "normal.f64",
             "prim": "prim.i32", "albedo": "albedo.f32"}
    got = {k: np.fromfile(tmp_path / f, ref[k].dtype).reshape(ref[k].shape)
           for k, f in files.items()}
    _same(got, ds.gbuffer())
    _same(got, ref)
    ppm = open(tmp_path / "depth.ppm", "rb").read()
    assert ppm.startswith(b"P6") and len(ppm) >= 37 * 21 * 3
