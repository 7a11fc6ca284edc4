"""The packet kernel's camera-cone mask table (csrc/rt_cone_table.hpp, packet_cone_table_kernel):
the two C2 variants (marching, RTAMD_PK_FIX=0, and fix-up, =1) read each wave tile's candidate
mask from a per-camera, per-launch-shape table instead of forming it in the wave.  Every frame
here is rendered with tables on and off (RTAMD_PK_CONE_TAB) through both variants and compared
bit for bit with the C oracle; rt_debug_cone_table proves which path ran.  Frames of 64x40, 9x7
and 193x109 pixels."""
import dataclasses
import math

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


def _scene(w, h, focal=None, name="cone"):
    return SceneData(Camera(CAM, w / 2.0 if focal is None else focal, w, h, 0.0, 200.0, 1),
                     name=name)


def _aim(sc, px, py, t):
    """The point at distance t on the camera ray through screen position (px, py) (pixel centres
    are the integers; the boundary between tiles is at 8k - 0.5)."""
    c = sc.camera
    v = np.array([px - c.width / 2.0 - c.position[0], c.height / 2.0 - py - c.position[1], c.focal])
    return np.array(c.position) + t * v / np.linalg.norm(v), t / np.linalg.norm(v)


def _room(sc):
    sc.add_plane((0.0, -10.0, 0.0), (0.0, 1.0, 0.0), Material((0.9, 0.9, 0.9)))
    sc.add_plane((0.0, 0.0, 15.0), (0.0, 0.0, -1.0), Material((0.7, 0.8, 0.9)))
    sc.add_light((3.0, 11.0, -12.0), (1.0, 1.0, 1.0), 300.0)
    return sc


def lattice(w, h):
    """Small spheres whose silhouettes cross tile corners and tile edges."""
    sc = _scene(w, h)
    spots = [(8 * i - 0.5, 8 * j - 0.5) for j in range(1, (h + 7) // 8) for i in range(1, (w + 7) // 8)]
    spots += [(8 * i + 3.5, 8 * j - 0.5) for j in range(1, (h + 7) // 8) for i in range((w + 7) // 8)]
    spots += [(8 * i - 0.5, 8 * j + 3.0) for j in range((h + 7) // 8) for i in range(1, (w + 7) // 8)]
    if not spots:
        spots = [(3.5, 3.5)]
    step = max(1, math.ceil(len(spots) / 60))
    for k, (px, py) in enumerate(spots[::step][:60]):
        p, pix = _aim(sc, px, py, 20.0 + (k % 7))
        sc.add_sphere(tuple(p), pix * (0.6 + 0.35 * (k % 5)), Material((0.9, 0.3 + 0.01 * k, 0.2)))
    return _room(sc)


def subpixel(w, h):
    """A sub-pixel sphere in the corner pixel of a tile, and one in the image's last pixel."""
    sc = _scene(w, h)
    for px, py in ((8 % w, 8 % h), (w - 1, h - 1), (7 % w, 0)):
        p, pix = _aim(sc, px, py, 18.0)
        sc.add_sphere(tuple(p), 0.3 * pix, Material((0.2, 0.9, 0.3)))
    return _room(sc)


def inside(w, h):
    """The camera inside one sphere and within 1.01 r of another."""
    sc = _scene(w, h)
    sc.add_sphere((1.0, -2.0, -20.0), 60.0, Material((0.4, 0.5, 0.9)))
    p, _ = _aim(sc, -10.0 * w, 0.6 * h, 1.005 * 3.0)  # off to the left: fills the left half
    sc.add_sphere(tuple(p), 3.0, Material((0.9, 0.8, 0.1)))
    p, pix = _aim(sc, 0.7 * w, 0.3 * h, 12.0)
    sc.add_sphere(tuple(p), 4.0 * pix, Material((0.9, 0.1, 0.1)))
    sc.add_light((0.0, 5.0, -20.0), (1.0, 1.0, 1.0), 200.0)
    return sc


def short_focal(w, h):
    """A focal length so short that the tiles' cones exceed 90 degrees."""
    sc = _scene(w, h, focal=0.05)
    for k, (x, y, z) in enumerate([(-6.0, 2.0, -24.0), (5.0, -3.0, -24.5), (0.0, 0.0, 5.0),
                                   (0.5, 0.2, -24.9), (20.0, 10.0, -25.0), (-1.0, 8.0, -26.0)]):
        sc.add_sphere((x, y, z), 0.05 + 0.6 * (k % 3), Material((0.3 + 0.1 * k, 0.6, 0.5)))
    return _room(sc)


def behind(w, h):
    """Every sphere behind the camera."""
    sc = _scene(w, h)
    for k in range(9):
        sc.add_sphere((-8.0 + 2.0 * k, -3.0 + k % 4, -30.0 - 3.0 * (k % 3)), 0.5 + 0.3 * (k % 4),
                      Material((0.5, 0.5, 0.9)))
    return _room(sc)


SCENES = {"lattice": lattice, "subpixel": subpixel, "inside": inside, "short_focal": short_focal,
          "behind": behind}


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


def _check_all_paths(ctx, oracle, monkeypatch, sc, plan=None, bias=1e-3, expect_table=True):
    """Two-frame batches of sc's camera, tables on / off x fix-up / marching variant, each on a
    fresh device scene (so each takes the ring): every frame is the oracle's."""
    plan = plan or {}
    w, h = sc.camera.width, sc.camera.height
    ref, _, _ = oracle.render(sc, bias=bias)
    ref8 = oracle.tonemap(ref, 1)
    rows = _plan_rows(h, plan)
    ref, ref8 = ref[rows], ref8.reshape(h, w, 3)[rows].reshape(-1)
    for tab in ("1", "0"):
        for fix in ("0", "1"):
            monkeypatch.setenv("RTAMD_PK_CONE_TAB", tab)
            monkeypatch.setenv("RTAMD_PK_FIX", fix)
            ds = ctx.scene(sc)
            try:
                opts = capi.default_opts(tonemap=1, bias=bias, **plan)
                assert capi.rendered_rows(opts, h) == len(rows)
                with0, without0 = ctx.debug_cone_table()
                got, got8 = _batch(ctx, ds, ds.cameras(np.repeat(ds.camera["position"], 2, axis=0)),
                                   opts, len(rows), w)
                with1, without1 = ctx.debug_cone_table()
            finally:
                ds.close()
            used = (with1 - with0, without1 - without0)
            assert used == ((2, 0) if tab == "1" and expect_table else (0, 2)), (tab, fix, used)
            for f in range(2):
                assert np.array_equal(got[f], ref), (tab, fix, f)
                assert np.array_equal(got8[f], ref8), (tab, fix, f)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", sorted(SCENES))
def test_scene_kinds_are_the_oracles(ctx, oracle, monkeypatch, kind, size):
    _check_all_paths(ctx, oracle, monkeypatch, SCENES[kind](*size))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("plan", ["b1_2x2", "3x3", "8x2"])
def test_row_plans_are_the_oracles_rows(ctx, oracle, monkeypatch, plan, size):
    _check_all_paths(ctx, oracle, monkeypatch, lattice(*size), plan=PLANS[plan])


@pytest.mark.parametrize("bias", [1e-3, 1e-12])
def test_bias(ctx, oracle, monkeypatch, bias):
    _check_all_paths(ctx, oracle, monkeypatch, lattice(193, 109), bias=bias)


def test_65_spheres_keep_the_in_kernel_cull(ctx, oracle, monkeypatch):
    """Tables serve the variants of up to 64 spheres: a 65-sphere scene renders as before."""
    sc = _scene(64, 40)
    for k in range(65):
        p, pix = _aim(sc, 1.0 + (k % 13) * 4.9, 1.0 + (k // 13) * 8.7, 15.0 + (k % 9))
        sc.add_sphere(tuple(p), pix * (0.7 + 0.2 * (k % 4)), Material((0.8, 0.4, 0.1 + 0.01 * k)))
    _check_all_paths(ctx, oracle, monkeypatch, _room(sc), expect_table=False)


def _moved(sc, pos):
    return dataclasses.replace(sc, camera=dataclasses.replace(sc.camera, position=tuple(pos)))


TAB_FIX = [("1", "0"), ("1", "1"), ("0", "0"), ("0", "1")]


def _used(ctx, before):
    a, b = ctx.debug_cone_table()
    return a - before[0], b - before[1]


@pytest.mark.parametrize("tab,fix", TAB_FIX)
def test_batch_of_five_cameras_ring_promotion_cache(ctx, oracle, monkeypatch, tab, fix):
    """One batch of five different cameras, three times: the tables are formed into the batch's
    ring entry, then into the cameras' new cache entries, then found there."""
    monkeypatch.setenv("RTAMD_PK_CONE_TAB", tab)
    monkeypatch.setenv("RTAMD_PK_FIX", fix)
    w, h = 193, 109
    sc = lattice(w, h)
    pos = [np.array(CAM) + d for d in ((0, 0, 0), (0.4, -0.3, 0.5), (-7.0, 2.0, -3.0),
                                       (30.0, -20.0, 1.0), (0.0, 0.0, 24.0))]
    refs = [oracle.render(_moved(sc, p))[0] for p in pos]
    ds = ctx.scene(sc)
    try:
        for rnd in range(3):
            before = ctx.debug_cone_table()
            got, _ = _batch(ctx, ds, ds.cameras(np.array(pos)), capi.default_opts(tonemap=1), h, w)
            assert _used(ctx, before) == ((5, 0) if tab == "1" else (0, 5)), rnd
            for f in range(5):
                assert np.array_equal(got[f], refs[f]), (rnd, f)
    finally:
        ds.close()


@pytest.mark.parametrize("tab,fix", TAB_FIX)
def test_one_camera_under_two_launch_shapes(ctx, oracle, monkeypatch, tab, fix):
    """One camera rendered alternately under two launch shapes: a table per shape."""
    monkeypatch.setenv("RTAMD_PK_CONE_TAB", tab)
    monkeypatch.setenv("RTAMD_PK_FIX", fix)
    w, h = 193, 109
    sc = lattice(w, h)
    ref, _, _ = oracle.render(sc)
    ds = ctx.scene(sc)
    try:
        cams = ds.cameras(np.repeat(ds.camera["position"], 2, axis=0))
        for rnd in range(6):
            plan = PLANS["3x3"] if rnd % 2 else PLANS["all"]
            rows = _plan_rows(h, plan)
            before = ctx.debug_cone_table()
            # (no tile-order recording launch: it takes the general variant, without tables)
            got, _ = _batch(ctx, ds, cams, capi.default_opts(
                tonemap=1, flags=capi.RT_FLAG_NO_TILE_ORDER, **plan), len(rows), w)
            assert _used(ctx, before) == ((2, 0) if tab == "1" else (0, 2)), rnd
            for f in range(2):
                assert np.array_equal(got[f], ref[rows]), (rnd, f)
    finally:
        ds.close()


def _focal(sc, focal):
    return dataclasses.replace(sc, camera=dataclasses.replace(sc.camera, focal=focal))


@pytest.mark.parametrize("batch", [False, True], ids=["one_frame", "batch"])
@pytest.mark.parametrize("tab,fix", TAB_FIX)
def test_one_position_at_two_focal_lengths(ctx, oracle, monkeypatch, tab, fix, batch):
    """A zoom: one camera position on one device scene rendered alternately at two focal
    lengths (the focal length is the render call's camera's, not the scene's).  The masks depend
    on it, so each focal length has a table of its own; every frame is the oracle's for its
    focal length.  One-frame launches (rt_render_device) and two-frame batches."""
    monkeypatch.setenv("RTAMD_PK_CONE_TAB", tab)
    monkeypatch.setenv("RTAMD_PK_FIX", fix)
    w, h = 193, 109
    sc = lattice(w, h)  # built for focal w / 2: at 3 w the spheres cover other tiles
    focals = (w / 2.0, 3.0 * w)
    refs = [oracle.render(_focal(sc, f))[0] for f in focals]
    assert not np.array_equal(refs[0], refs[1])
    ds = ctx.scene(sc)
    try:
        used = []
        for rnd in range(8):
            k = rnd % 2
            ds.camera["focal"] = focals[k]
            before = ctx.debug_cone_table()
            opts = capi.default_opts(tonemap=1, flags=capi.RT_FLAG_NO_TILE_ORDER)
            if batch:
                got, _ = _batch(ctx, ds, ds.cameras(np.repeat(ds.camera["position"], 2, axis=0)),
                                opts, h, w)
            else:
                h64 = torch.full((h * w * 3,), -1.0, dtype=torch.float64, device="cuda")
                ds.render_device(h64.data_ptr(), None, None, opts)
                ctx.synchronize()
                got = h64.cpu().numpy().reshape(1, h, w, 3)
            used.append(_used(ctx, before))
            for f in range(len(got)):
                assert np.array_equal(got[f], refs[k]), (rnd, f)
        n = 2 if batch else 1
        if tab == "0":
            assert used == [(0, n)] * 8
        elif batch:
            assert used == [(n, 0)] * 8
        else:  # the first sighting of the position takes the publish slot, without a table
            assert used == [(0, 1)] + [(1, 0)] * 7
    finally:
        ds.close()


@pytest.mark.parametrize("tab,fix", TAB_FIX)
def test_table_with_a_built_tile_order(ctx, oracle, monkeypatch, tab, fix):
    """Static-camera batches with the default flags: ring, promotion, then the launch that
    records the wave durations (the general variant: no table), then the launches after the
    tile order is built, which dispatch by it when the costs are wide.  The table is indexed by
    tile, not by dispatch position, so every frame stays the oracle's either way."""
    monkeypatch.setenv("RTAMD_PK_CONE_TAB", tab)
    monkeypatch.setenv("RTAMD_PK_FIX", fix)
    w, h = 193, 109
    sc = lattice(w, h)
    ref, _, _ = oracle.render(sc)
    ds = ctx.scene(sc)
    try:
        cams = ds.cameras(np.repeat(ds.camera["position"], 2, axis=0))
        used = []
        for rnd in range(6):
            before = ctx.debug_cone_table()
            got, _ = _batch(ctx, ds, cams, capi.default_opts(tonemap=1), h, w)
            used.append(_used(ctx, before))
            for f in range(2):
                assert np.array_equal(got[f], ref), (rnd, f)
        state, order, _ = ds.debug_tile_order()
        assert state == 2  # the order was built from the recording launch
        print("tile order differs from the default:", order is not None and
              not np.array_equal(order, np.sort(order)))
        if tab == "1":
            assert used == [(2, 0), (2, 0), (0, 2), (2, 0), (2, 0), (2, 0)]
        else:
            assert used == [(0, 2)] * 6
    finally:
        ds.close()


def test_one_frame_launches(ctx, oracle, monkeypatch):
    """A one-frame launch of a camera seen for the first time gets no table (one more launch per
    frame costs more than it saves); from its second sighting on it has one."""
    monkeypatch.setenv("RTAMD_PK_CONE_TAB", "1")
    monkeypatch.setenv("RTAMD_PK_FIX", "0")
    w, h = 64, 40
    sc = lattice(w, h)
    ref, _, _ = oracle.render(sc)
    ds = ctx.scene(sc)
    try:
        used = []
        for rnd in range(3):
            before = ctx.debug_cone_table()
            # (no tile-order recording launch: it takes the general variant, without tables)
            out = ds.render(hdr64=True, opts=capi.default_opts(flags=capi.RT_FLAG_NO_TILE_ORDER))
            used.append(_used(ctx, before))
            assert np.array_equal(out["hdr64"], ref), rnd
        assert used == [(0, 1), (1, 0), (1, 0)]
    finally:
        ds.close()
