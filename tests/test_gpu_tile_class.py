"""The packet kernel's tile class words (tile_class_word in csrc/rt_shadow_table.hpp, formed by
packet_cone_table_kernel after the cone and shadow words): the fix-up variant of C2's kernel
renders a tile that sees one plane or only sky, and whose shadow words are all zero, on a uniform
path (pk_uniform_tile) that reads no LDS image, and a workgroup of such tiles skips the image
staging.  Frames are the same bits either way, so every frame here is rendered with
RTAMD_PK_TILE_CLASS 1 and 0 through the fix-up (RTAMD_PK_FIX=1) and the marching (=0, general
path only) variant — as a batch of two camera positions (ring tables), as a batch of one cached
position and as one-frame launches of a cached camera — and compared bit for bit with the C
oracle; rt_debug_tile_class shows which frames had class words.

Uniform tiles of the scenes, counted on the CPU with the header's functions (two waves side by
side per workgroup):
    room         64x40: 23 of 40 tiles, 11 whole workgroups and a mixed one; 9x7: none (general
                 path with lanes past the edge); 193x109: 297 of 364
    horizon      64x40: 16, all sky; 193x109: 202, of them 156 sky
    near_lights  64x40: 11; 193x109: 231, with undecided rows that must still reach the fix-up
    below_floor  64x40: 26; 9x7: 2 tiles, one workgroup, most lanes past the edge
    three_lights 64x40: 3
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from raytracingengine_amd import capi
from raytracingengine_amd.scene import Camera, Material, SceneData

pytestmark = pytest.mark.gpu

SIZES = [(64, 40), (9, 7), (193, 109)]
PLANS = {"all": {}, "b1_2x2": dict(row_begin=1, row_block=2, row_cycle=2),
         "3x3": dict(row_block=3, row_cycle=3), "8x2": dict(row_block=8, row_cycle=2)}
CAM = (0.0, 0.0, -25.0)
SECOND = (0.7, -0.4, -22.5)
BIAS = 1e-3
GREY, BLUE, RED = Material((0.9, 0.9, 0.9)), Material((0.7, 0.8, 0.9)), Material((0.9, 0.3, 0.2))
# (RTAMD_PK_TILE_CLASS, RTAMD_PK_FIX)
SWITCHES = [("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")]


def _scene(w, h, cam=CAM, focal=None):
    return SceneData(Camera(cam, w / 2.0 if focal is None else focal, w, h, 0.0, 200.0, 1),
                     name="tile_class")


def _floor_wall(sc):
    sc.add_plane((0.0, -10.0, 0.0), (0.0, 1.0, 0.0), GREY)
    sc.add_plane((0.0, 0.0, 15.0), (0.0, 0.0, -1.0), BLUE)
    return sc


def room(w, h):
    """Floor and back wall, a sphere standing on the floor and one floating."""
    sc = _floor_wall(_scene(w, h))
    sc.add_sphere((-4.0, -8.5, 4.0), 1.5, RED)
    sc.add_sphere((5.0, -4.0, 9.0), 1.0, RED)
    sc.add_light((3.0, 11.0, -12.0), (1.0, 1.0, 1.0), 300.0)
    return sc


def horizon(w, h):
    """A floor under the sky: its horizon crosses the middle tile row; the rows above are sky."""
    sc = _scene(w, h)
    sc.add_plane((0.0, -10.0, 0.0), (0.0, 1.0, 0.0), GREY)
    sc.add_sphere((-30.0, -7.0, 20.0), 3.0, RED)
    sc.add_sphere((2.0, -9.5, -5.0), 0.5, RED)
    sc.add_light((-60.0, 0.0, 30.0), (1.0, 1.0, 1.0), 900.0)
    return sc


def near_lights(w, h):
    """A light within 2·bias of the floor, one within 2·bias of the wall and one behind the wall:
    plane hits next to them are undecided and go to the fix-up."""
    sc = _floor_wall(_scene(w, h))
    sc.add_sphere((-3.0, -10.0 + 1.2 * BIAS + 0.4, 0.0), 0.4, RED)
    sc.add_sphere((4.0, -2.0, 15.0 - 0.3 - BIAS), 0.3, RED)
    sc.add_light((6.0, -10.0 + 1.5 * BIAS, -3.0), (1.0, 1.0, 1.0), 60.0)
    sc.add_light((-6.0, 3.0, 15.0 - 1.9 * BIAS), (1.0, 0.9, 0.8), 60.0)
    sc.add_light((0.0, 5.0, 25.0), (1.0, 1.0, 1.0), 300.0)
    return sc


def below_floor(w, h):
    """The camera below the floor: the planes' shading normals flip."""
    sc = _floor_wall(_scene(w, h, cam=(1.0, -22.0, -25.0)))
    sc.add_sphere((0.0, -13.0, 0.0), 1.5, RED)
    sc.add_sphere((-5.0, -11.0, 6.0), 1.0, RED)
    sc.add_light((2.0, -30.0, -5.0), (1.0, 1.0, 1.0), 300.0)
    sc.add_light((2.0, 8.0, -5.0), (1.0, 1.0, 1.0), 300.0)
    return sc


def three_lights(w, h):
    sc = _floor_wall(_scene(w, h))
    for k, (x, y, z, r) in enumerate([(-4.0, -8.5, 4.0, 1.5), (5.0, -4.0, 9.0, 1.0),
                                      (0.0, 3.0, 12.0, 2.0), (8.0, -9.2, -2.0, 0.8)]):
        sc.add_sphere((x, y, z), r, Material((0.9, 0.3 + 0.1 * k, 0.2)))
    sc.add_light((3.0, 11.0, -12.0), (1.0, 1.0, 1.0), 150.0)
    sc.add_light((-9.0, 4.0, 2.0), (1.0, 0.8, 0.8), 100.0)
    sc.add_light((12.0, -6.0, 10.0), (0.8, 0.8, 1.0), 100.0)
    return sc


def no_lights(w, h):
    sc = _floor_wall(_scene(w, h))
    sc.add_sphere((-4.0, -8.5, 4.0), 1.5, RED)
    return sc


def spheres64(w, h):
    """One sphere past the shadow table's 63: cone masks only, so no class words."""
    sc = _floor_wall(_scene(w, h))
    for k in range(64):
        sc.add_sphere((-10.5 + 3.0 * (k % 8), -9.6 + 0.8 * (k % 3), -8.0 + 2.8 * (k // 8)),
                      0.35 + 0.05 * (k % 4), Material((0.8, 0.4, 0.1 + 0.01 * k)))
    sc.add_light((3.0, 11.0, -12.0), (1.0, 1.0, 1.0), 300.0)
    return sc


SCENES = {"room": room, "horizon": horizon, "near_lights": near_lights,
          "below_floor": below_floor, "three_lights": three_lights, "no_lights": no_lights,
          "spheres64": spheres64}


def _moved(sc, pos):
    return dataclasses.replace(sc, camera=dataclasses.replace(sc.camera, position=tuple(pos)))


@functools.lru_cache(maxsize=None)
def _reference(kind, size, pos, focal, bias, max_rec):
    """The oracle's frame and Reinhard bytes, computed once per frame and shared (read-only)."""
    from oracle import pyoracle
    sc = SCENES[kind](*size)
    cam = dataclasses.replace(sc.camera, position=tuple(pos if pos else sc.camera.position),
                              focal=focal if focal else sc.camera.focal)
    sc = dataclasses.replace(sc, camera=cam)
    ref, _, _ = pyoracle.render(sc, max_recursion=max_rec, bias=bias)
    ref8 = pyoracle.tonemap(ref, 1).reshape(size[1], size[0], 3)
    ref.setflags(write=False)
    ref8.setflags(write=False)
    return ref, ref8


def _plan_rows(h, plan):
    o = capi.default_opts(**plan)
    b0 = o.row_begin
    if o.row_cycle <= 1 or o.row_block == 0:
        return list(range(b0, h))
    rows = []
    for b in range(b0, h, o.row_block * o.row_cycle):
        rows += list(range(b, min(b + o.row_block, h)))
    return rows


def _batch(ctx, ds, cams, opts, rows, w):
    n = len(cams)
    h64 = torch.full((n * rows * w * 3,), -1.0, dtype=torch.float64, device="cuda")
    l8 = torch.zeros(n * rows * w * 3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ds.render_batch(cams, h64.data_ptr(), None, l8.data_ptr(), opts)
    ctx.synchronize()
    return h64.cpu().numpy().reshape(n, rows, w, 3), l8.cpu().numpy().reshape(n, rows, w, 3)


def _used(ctx, before):
    return tuple(np.array(ctx.debug_tile_class()) - before)


def _check_all_paths(ctx, monkeypatch, kind, size, plan=None, words=True, max_rec=10):
    """Under the four switch combinations, each on a fresh device scene: a batch of two camera
    positions (the batch ring's tables), the first position twice (by then a cached camera with
    tables of its own) and three one-frame launches of it."""
    plan = plan or {}
    w, h = size
    sc = SCENES[kind](w, h)
    rows = _plan_rows(h, plan)
    pos = [tuple(sc.camera.position), SECOND]
    refs = [_reference(kind, size, p, None, BIAS, max_rec) for p in pos]
    for cls, fix in SWITCHES:
        monkeypatch.setenv("RTAMD_PK_TILE_CLASS", cls)
        monkeypatch.setenv("RTAMD_PK_FIX", fix)
        want = (lambda n: (n, 0)) if cls == "1" and words else (lambda n: (0, n))
        ds = ctx.scene(sc)
        try:
            # (no tile order: a launch that records wave durations takes the general variant)
            opts = capi.default_opts(tonemap=1, bias=BIAS, max_recursion=max_rec,
                                     flags=capi.RT_FLAG_NO_TILE_ORDER, **plan)
            assert capi.rendered_rows(opts, h) == len(rows)
            for cams in (pos, [pos[0], pos[0]], [pos[0], pos[0]]):
                before = np.array(ctx.debug_tile_class())
                got, got8 = _batch(ctx, ds, ds.cameras(np.array(cams, np.float64)), opts,
                                   len(rows), w)
                assert _used(ctx, before) == want(2), (cls, fix, cams)
                for f, p in enumerate(cams):
                    ref, ref8 = refs[pos.index(p)]
                    assert np.array_equal(got[f], ref[rows]), (cls, fix, cams, f)
                    assert np.array_equal(got8[f], ref8[rows]), (cls, fix, cams, f)
            for k in range(3):  # one-frame launches (the marching variant), the camera cached
                before = np.array(ctx.debug_tile_class())
                out = ds.render(hdr64=True, tonemap=1, opts=opts)
                if k == 2:
                    assert _used(ctx, before) == want(1), (cls, fix)
                assert np.array_equal(out["hdr64"], refs[0][0][rows]), (cls, fix, k)
                assert np.array_equal(out["ldr"], refs[0][1][rows]), (cls, fix, k)
        finally:
            ds.close()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["below_floor", "horizon", "near_lights", "room", "three_lights"])
def test_scene_kinds_are_the_oracles(ctx, monkeypatch, kind, size):
    _check_all_paths(ctx, monkeypatch, kind, size)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("plan", ["b1_2x2", "3x3", "8x2"])
def test_row_plans_are_the_oracles_rows(ctx, monkeypatch, plan, size):
    _check_all_paths(ctx, monkeypatch, "room", size, plan=PLANS[plan])


def test_no_recursion_is_all_sky(ctx, monkeypatch):
    """max_recursion 0: every pixel is the sky colour, and no workgroup may skip anything it
    needs (the class words are ignored)."""
    _check_all_paths(ctx, monkeypatch, "room", (64, 40), max_rec=0, words=False)


def test_no_light_has_no_class_words(ctx, monkeypatch):
    """Without a point light there is no shadow table, so no class words either."""
    _check_all_paths(ctx, monkeypatch, "no_lights", (64, 40), words=False)


def test_64_spheres_render_without_class_words(ctx, monkeypatch):
    _check_all_paths(ctx, monkeypatch, "spheres64", (64, 40), words=False)


@pytest.mark.parametrize("cone,shadow,cls,with_words",
                         [("1", "1", "1", True), ("1", "1", "0", False), ("0", "1", "1", False),
                          ("1", "0", "1", False), ("0", "0", "1", False)])
def test_class_words_need_both_tables_and_the_switch(ctx, monkeypatch, cone, shadow, cls,
                                                      with_words):
    monkeypatch.setenv("RTAMD_PK_CONE_TAB", cone)
    monkeypatch.setenv("RTAMD_PK_SHADOW_TAB", shadow)
    monkeypatch.setenv("RTAMD_PK_TILE_CLASS", cls)
    monkeypatch.setenv("RTAMD_PK_FIX", "1")
    size = (64, 40)
    sc = room(*size)
    ref, ref8 = _reference("room", size, None, None, BIAS, 10)
    ds = ctx.scene(sc)
    try:
        cams = ds.cameras(np.array([sc.camera.position, SECOND], np.float64))
        before = np.array(ctx.debug_tile_class())
        got, got8 = _batch(ctx, ds, cams, capi.default_opts(tonemap=1, bias=BIAS), size[1],
                           size[0])
        assert _used(ctx, before) == ((2, 0) if with_words else (0, 2))
        assert np.array_equal(got[0], ref) and np.array_equal(got8[0], ref8)
    finally:
        ds.close()


@pytest.mark.parametrize("cls,fix", SWITCHES)
def test_one_position_at_two_focal_lengths(ctx, monkeypatch, cls, fix):
    """A zoom: one position on one device scene rendered alternately at two focal lengths.  The
    class words depend on the focal length like the masks: each has a table of its own."""
    monkeypatch.setenv("RTAMD_PK_TILE_CLASS", cls)
    monkeypatch.setenv("RTAMD_PK_FIX", fix)
    size = (193, 109)
    w, h = size
    sc = room(w, h)
    focals = (w / 2.0, 1.5 * w)
    refs = [_reference("room", size, None, f, BIAS, 10)[0] for f in focals]
    assert not np.array_equal(refs[0], refs[1])
    ds = ctx.scene(sc)
    try:
        for rnd in range(6):
            k = rnd % 2
            ds.camera["focal"] = focals[k]
            before = np.array(ctx.debug_tile_class())
            got, _ = _batch(ctx, ds, ds.cameras(np.repeat(ds.camera["position"], 2, axis=0)),
                            capi.default_opts(tonemap=1, bias=BIAS,
                                              flags=capi.RT_FLAG_NO_TILE_ORDER), h, w)
            assert _used(ctx, before) == ((2, 0) if cls == "1" else (0, 2)), rnd
            for f in range(2):
                assert np.array_equal(got[f], refs[k]), (rnd, f)
    finally:
        ds.close()


@pytest.mark.parametrize("cls,fix", SWITCHES)
def test_one_scene_at_two_biases(ctx, monkeypatch, cls, fix):
    """One device scene and camera at a small bias until its table is cached, then at a large
    one, then at the small one again.  The class rests on the shadow words, which depend on the
    bias: each bias has a table of its own, and every frame is the oracle's for its bias."""
    monkeypatch.setenv("RTAMD_PK_TILE_CLASS", cls)
    monkeypatch.setenv("RTAMD_PK_FIX", fix)
    size = (193, 109)
    w, h = size
    big = 0.9  # (under 1: directLightning drops a light whose transmittance is <= bias)
    sc = room(w, h)
    refs = {b: _reference("room", size, None, None, b, 10)[0] for b in (BIAS, big)}
    assert not np.array_equal(refs[BIAS], refs[big])
    ds = ctx.scene(sc)
    try:
        cams = ds.cameras(np.repeat(ds.camera["position"], 2, axis=0))
        for rnd, b in enumerate([BIAS, BIAS, BIAS, big, big, BIAS, big]):
            before = np.array(ctx.debug_tile_class())
            got, _ = _batch(ctx, ds, cams, capi.default_opts(
                tonemap=1, bias=b, flags=capi.RT_FLAG_NO_TILE_ORDER), h, w)
            assert _used(ctx, before) == ((2, 0) if cls == "1" else (0, 2)), rnd
            for f in range(2):
                assert np.array_equal(got[f], refs[b]), (rnd, b, f)
    finally:
        ds.close()
