"""The packet kernel's shadow-cull mask table (csrc/rt_shadow_table.hpp, formed by
packet_cone_table_kernel next to the camera-cone masks): the two C2 variants (marching,
RTAMD_PK_FIX=0, and fix-up, =1) read a tile's candidate mask for each light from a per-camera,
per-launch-shape table instead of forming it in the wave with origin_ball + cull_capsule.  Every
frame here is rendered under the four combinations of RTAMD_PK_CONE_TAB and RTAMD_PK_SHADOW_TAB
through both variants and compared bit for bit with the C oracle; rt_debug_shadow_table and
rt_debug_cone_table prove which path ran.  Frames of 64x40, 9x7 and 193x109 pixels."""
import dataclasses

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
BIAS = 1e-3
GREY, BLUE, RED = Material((0.9, 0.9, 0.9)), Material((0.7, 0.8, 0.9)), Material((0.9, 0.3, 0.2))
# (RTAMD_PK_CONE_TAB, RTAMD_PK_SHADOW_TAB)
SWITCHES = [("1", "1"), ("1", "0"), ("0", "1"), ("0", "0")]


def _scene(w, h, cam=CAM, focal=None):
    return SceneData(Camera(cam, w / 2.0 if focal is None else focal, w, h, 0.0, 200.0, 1),
                     name="shadow")


def _floor_wall(sc):
    sc.add_plane((0.0, -10.0, 0.0), (0.0, 1.0, 0.0), GREY)
    sc.add_plane((0.0, 0.0, 15.0), (0.0, 0.0, -1.0), BLUE)
    return sc


def room(w, h):
    """Floor and back wall; a sphere standing on the floor and one floating, whose shadows fall
    across several tiles that see planes only.  (The floor/wall edge crosses one tile row, where
    both planes are visible and neither hides the other.)"""
    sc = _floor_wall(_scene(w, h))
    sc.add_sphere((-4.0, -8.5, 4.0), 1.5, RED)
    sc.add_sphere((5.0, -4.0, 9.0), 1.0, RED)
    sc.add_light((3.0, 11.0, -12.0), (1.0, 1.0, 1.0), 300.0)
    return sc


def horizon(w, h):
    """A floor under the sky: its horizon crosses the middle tile row, which gets no word; a
    sphere beyond the image's left edge shadows the floor in view."""
    sc = _scene(w, h)
    sc.add_plane((0.0, -10.0, 0.0), (0.0, 1.0, 0.0), GREY)
    sc.add_sphere((-30.0, -7.0, 20.0), 3.0, RED)
    sc.add_sphere((2.0, -9.5, -5.0), 0.5, RED)
    sc.add_light((-60.0, 0.0, 30.0), (1.0, 1.0, 1.0), 900.0)
    return sc


def near_lights(w, h):
    """A light within 2·bias of the floor, one within 2·bias of the wall and one behind the wall."""
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
    """(Two planes: scenes of three or more take the plane-culling variant, which reads no table.)"""
    sc = _floor_wall(_scene(w, h))
    for k, (x, y, z, r) in enumerate([(-4.0, -8.5, 4.0, 1.5), (5.0, -4.0, 9.0, 1.0),
                                      (0.0, 3.0, 12.0, 2.0), (8.0, -9.2, -2.0, 0.8)]):
        sc.add_sphere((x, y, z), r, Material((0.9, 0.3 + 0.1 * k, 0.2)))
    sc.add_light((3.0, 11.0, -12.0), (1.0, 1.0, 1.0), 150.0)
    sc.add_light((-9.0, 4.0, 2.0), (1.0, 0.8, 0.8), 100.0)
    sc.add_light((12.0, -6.0, 10.0), (0.8, 0.8, 1.0), 100.0)
    return sc


def many(n):
    def build(w, h):
        """n small spheres in a grid over the floor, up to the table's 63 and one past it."""
        sc = _floor_wall(_scene(w, h))
        for k in range(n):
            sc.add_sphere((-10.5 + 3.0 * (k % 8), -9.6 + 0.8 * (k % 3), -8.0 + 2.8 * (k // 8)),
                          0.35 + 0.05 * (k % 4), Material((0.8, 0.4, 0.1 + 0.01 * k)))
        sc.add_light((3.0, 11.0, -12.0), (1.0, 1.0, 1.0), 300.0)
        return sc
    return build


SCENES = {"room": room, "horizon": horizon, "near_lights": near_lights,
          "below_floor": below_floor, "three_lights": three_lights, "spheres63": many(63)}


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
    return h64.cpu().numpy().reshape(n, rows, w, 3), l8.cpu().numpy().reshape(n, -1)


def _counts(ctx):
    return np.array(ctx.debug_cone_table() + ctx.debug_shadow_table())


def _expected(cone, shadow, n, shadow_table=True):
    c = (n, 0) if cone == "1" else (0, n)
    s = (n, 0) if shadow == "1" and shadow_table else (0, n)
    return c + s


def _moved(sc, pos):
    return dataclasses.replace(sc, camera=dataclasses.replace(sc.camera, position=tuple(pos)))


def _check_all_paths(ctx, oracle, monkeypatch, sc, plan=None, shadow_table=True, second=None):
    """Two-frame batches — sc's camera twice, or with `second` as the other position — under the
    four switch combinations x fix-up / marching variant, each on a fresh device scene (so each
    takes the batch ring): every frame is the oracle's."""
    plan = plan or {}
    w, h = sc.camera.width, sc.camera.height
    rows = _plan_rows(h, plan)
    pos = [sc.camera.position, sc.camera.position if second is None else second]
    refs, refs8 = [], []
    for p in pos if second is not None else pos[:1]:
        ref, _, _ = oracle.render(_moved(sc, p), bias=BIAS)
        refs.append(ref[rows])
        refs8.append(oracle.tonemap(ref, 1).reshape(h, w, 3)[rows].reshape(-1))
    for cone, shadow in SWITCHES:
        for fix in ("0", "1"):
            monkeypatch.setenv("RTAMD_PK_CONE_TAB", cone)
            monkeypatch.setenv("RTAMD_PK_SHADOW_TAB", shadow)
            monkeypatch.setenv("RTAMD_PK_FIX", fix)
            ds = ctx.scene(sc)
            try:
                opts = capi.default_opts(tonemap=1, bias=BIAS, **plan)
                assert capi.rendered_rows(opts, h) == len(rows)
                before = _counts(ctx)
                got, got8 = _batch(ctx, ds, ds.cameras(np.array(pos, np.float64)), opts,
                                   len(rows), w)
                used = tuple(_counts(ctx) - before)
            finally:
                ds.close()
            assert used == _expected(cone, shadow, 2, shadow_table), (cone, shadow, fix, used)
            for f in range(2):
                assert np.array_equal(got[f], refs[f % len(refs)]), (cone, shadow, fix, f)
                assert np.array_equal(got8[f], refs8[f % len(refs8)]), (cone, shadow, fix, f)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", sorted(SCENES))
def test_scene_kinds_are_the_oracles(ctx, oracle, monkeypatch, kind, size):
    _check_all_paths(ctx, oracle, monkeypatch, SCENES[kind](*size))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_64_spheres_render_without_a_shadow_table(ctx, oracle, monkeypatch, size):
    """All ones must stay free to say "no word": a 64-sphere scene gets cone masks only."""
    _check_all_paths(ctx, oracle, monkeypatch, many(64)(*size), shadow_table=False)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("plan", ["b1_2x2", "3x3", "8x2"])
def test_row_plans_are_the_oracles_rows(ctx, oracle, monkeypatch, plan, size):
    _check_all_paths(ctx, oracle, monkeypatch, three_lights(*size), plan=PLANS[plan])


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_two_camera_positions_take_the_batch_ring(ctx, oracle, monkeypatch, size):
    _check_all_paths(ctx, oracle, monkeypatch, room(*size), second=(0.7, -0.4, -22.5))


@pytest.mark.parametrize("cone,shadow", SWITCHES)
@pytest.mark.parametrize("fix", ["0", "1"])
def test_one_position_at_two_focal_lengths(ctx, oracle, monkeypatch, cone, shadow, fix):
    """A zoom: one position on one device scene rendered alternately at two focal lengths.  The
    words depend on the focal length, so each has a table of its own (the cone table's key)."""
    monkeypatch.setenv("RTAMD_PK_CONE_TAB", cone)
    monkeypatch.setenv("RTAMD_PK_SHADOW_TAB", shadow)
    monkeypatch.setenv("RTAMD_PK_FIX", fix)
    w, h = 193, 109
    sc = three_lights(w, h)
    focals = (w / 2.0, 1.5 * w)
    refs = [oracle.render(dataclasses.replace(
        sc, camera=dataclasses.replace(sc.camera, focal=f)), bias=BIAS)[0] for f in focals]
    assert not np.array_equal(refs[0], refs[1])
    ds = ctx.scene(sc)
    try:
        for rnd in range(6):
            k = rnd % 2
            ds.camera["focal"] = focals[k]
            before = _counts(ctx)
            got, _ = _batch(ctx, ds, ds.cameras(np.repeat(ds.camera["position"], 2, axis=0)),
                            capi.default_opts(tonemap=1, bias=BIAS,
                                              flags=capi.RT_FLAG_NO_TILE_ORDER), h, w)
            assert tuple(_counts(ctx) - before) == _expected(cone, shadow, 2), rnd
            for f in range(2):
                assert np.array_equal(got[f], refs[k]), (rnd, f)
    finally:
        ds.close()


def bias_scene(w, h, big):
    """A wall seen through a long focal length (tiles smaller than `big`), a light off to the right
    about 1.5·big above the wall, and a sphere out of sight on the shadow rays that start `big`
    above the wall: words formed for a small bias leave it out, the rays at bias `big` meet it."""
    sc = _scene(w, h, focal=4.0 * w)
    sc.add_plane((0.0, 0.0, 15.0), (0.0, 0.0, -1.0), BLUE)
    sc.add_sphere((8.0, 0.0, 15.0 - big - 1.5 * big * (8.0 / 14.0)), 0.2 * big, RED)
    sc.add_sphere((9.0, 1.5, 15.0 - 0.5), 0.5, RED)
    sc.add_light((14.0, 0.0, 15.0 - 1.5 * big), (1.0, 1.0, 1.0), 300.0)
    return sc


@pytest.mark.parametrize("cone,shadow", SWITCHES)
@pytest.mark.parametrize("fix", ["0", "1"])
def test_one_scene_at_two_biases(ctx, oracle, monkeypatch, cone, shadow, fix):
    """One device scene and camera rendered at a small bias until its table is cached, then at a
    large one, then at the small one again.  The shadow words depend on the render call's bias
    (it enters every ball's radius), so each bias has a table of its own (the key carries it);
    every frame is the oracle's for its bias."""
    monkeypatch.setenv("RTAMD_PK_CONE_TAB", cone)
    monkeypatch.setenv("RTAMD_PK_SHADOW_TAB", shadow)
    monkeypatch.setenv("RTAMD_PK_FIX", fix)
    w, h = 193, 109
    big = 0.9  # (under 1: directLightning drops a light whose transmittance is <= bias)
    sc = bias_scene(w, h, big)
    refs = {b: oracle.render(sc, bias=b)[0] for b in (BIAS, big)}
    assert not np.array_equal(refs[BIAS], refs[big])
    # the sphere shadows the wall at the large bias only
    assert (refs[big].sum(axis=2) == 0.0).sum() > (refs[BIAS].sum(axis=2) == 0.0).sum()
    ds = ctx.scene(sc)
    try:
        cams = ds.cameras(np.repeat(ds.camera["position"], 2, axis=0))
        for rnd, b in enumerate([BIAS, BIAS, BIAS, big, big, BIAS, big]):
            before = _counts(ctx)
            got, _ = _batch(ctx, ds, cams, capi.default_opts(
                tonemap=1, bias=b, flags=capi.RT_FLAG_NO_TILE_ORDER), h, w)
            assert tuple(_counts(ctx) - before) == _expected(cone, shadow, 2), rnd
            for f in range(2):
                assert np.array_equal(got[f], refs[b]), (rnd, b, f)
    finally:
        ds.close()
