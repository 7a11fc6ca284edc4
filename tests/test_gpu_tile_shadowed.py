"""The split launch's third kernel: tiles that see one plane and whose shadow rays can meet a sphere
(tile_shadowed_mark in csrc/rt_shadow_table.hpp) are marked in their class words, filed in a list
of their own by packet_cone_table_kernel and rendered by packet_uniform_kernel<true>, which runs
the sphere block of the shadow classification over the tile's shadow words before the kept planes'.
Frames are the same bits either way, so every scene here is rendered through the fix-up variant
(RTAMD_PK_FIX=1) under RTAMD_PK_TILE_SHADOWED, RTAMD_PK_TILE_SPLIT and RTAMD_PK_PLANE_CLEAR, each
unset and 0, and compared bit for bit with the C oracle (float64 HDR, exact float32, Reinhard
bytes) and across the switches.  Each case renders its cameras three times on a fresh device
scene: a first sighting (ring tables, one launch), the launch that forms the cameras' cached tables
and lists (one launch: the host has no counts yet) and the split launch, whose use
rt_debug_tile_split and rt_debug_tile_shadowed show; the latter also shows that the scene has
shadowed tiles (a count of 0 skips the launch).

Sizes: 64x40, 100x60 (13 x 8 tiles: an odd tile column and a last tile row of 4 pixel rows, so
tiles reach past the right and bottom edges), 200x120, and one row plan (blocks of 8 rows, every
second block).
"""
import dataclasses
import functools

import numpy as np
import pytest

import test_gpu_tile_class as tc
from raytracingengine_amd import capi
from raytracingengine_amd.scene import Material

pytestmark = pytest.mark.gpu

SIZES = [(64, 40), (100, 60), (200, 120)]
BIAS = tc.BIAS
GREY, BLUE, RED = tc.GREY, tc.BLUE, tc.RED
SWITCHES = [(sh, sp, cl) for sh in (None, "0") for sp in (None, "0") for cl in (None, "0")]


def _floor(sc):
    sc.add_plane((0.0, -10.0, 0.0), (0.0, 1.0, 0.0), GREY)
    return sc


def one_sphere(w, h):
    """One sphere floating over a floor, the light above it."""
    sc = _floor(tc._scene(w, h))
    sc.add_sphere((0.0, -5.0, 5.0), 1.5, RED)
    sc.add_light((1.0, 15.0, 4.0), (1.0, 1.0, 1.0), 500.0)
    return sc


def wall_line(w, h):
    """Floor and back wall; the shadow runs over the floor and up the wall, across their line."""
    sc = tc._floor_wall(tc._scene(w, h))
    sc.add_sphere((-6.0, -2.0, 8.0), 1.5, RED)
    sc.add_light((-14.0, 6.0, 2.0), (1.0, 1.0, 1.0), 600.0)
    return sc


def sixteen(w, h):
    """16 small spheres close together over the floor: tiles under them keep three and more."""
    sc = _floor(tc._scene(w, h))
    for k in range(16):
        sc.add_sphere((-2.1 + 1.4 * (k % 4), -7.0 + 0.3 * (k % 3), 2.0 + 1.4 * (k // 4)), 0.5,
                      Material((0.9, 0.3 + 0.03 * k, 0.2)))
    sc.add_light((0.0, 14.0, 4.0), (1.0, 1.0, 1.0), 500.0)
    return sc


def four_lights(w, h):
    """Four lights around two spheres: a tile's four words differ, some of them zero."""
    sc = tc._floor_wall(tc._scene(w, h))
    sc.add_sphere((-5.0, -7.0, 3.0), 1.5, RED)
    sc.add_sphere((6.0, -3.0, 10.0), 1.2, RED)
    sc.add_light((-12.0, 6.0, 0.0), (1.0, 0.9, 0.9), 200.0)
    sc.add_light((12.0, 8.0, 2.0), (0.9, 1.0, 0.9), 200.0)
    sc.add_light((0.0, 12.0, 12.0), (0.9, 0.9, 1.0), 200.0)
    sc.add_light((2.0, -4.0, -20.0), (1.0, 1.0, 1.0), 200.0)
    return sc


def light_behind_camera(w, h):
    sc = _floor(tc._scene(w, h))
    sc.add_sphere((2.0, -4.0, 0.0), 1.0, RED)
    sc.add_light((32.0, 12.0, -45.0), (1.0, 1.0, 1.0), 4000.0)
    return sc


def small_sphere(w, h):
    """A small sphere just over the floor under its light: its shadow is smaller than a tile, so
    the tiles around it have the sphere in their word and no ray of theirs meets it."""
    sc = _floor(tc._scene(w, h))
    sc.add_sphere((2.0, -9.0, -5.0), 0.2, RED)
    sc.add_light((2.0, 11.0, -5.0), (1.0, 1.0, 1.0), 500.0)
    return sc


def light_in_sphere(w, h):
    """A sphere above the view with the light on its lowest point, the side facing the floor:
    every shadow ray of the floor enters the sphere at the light, at |L − so| = dist − bias·cos θ
    for a ray θ off the vertical, against max_dist = dist − bias: within the classification's
    margin Δ ≈ 8e-5 for θ up to ~20°, so those pixels are undecided and go through the fix-up
    launch.  (With the light `bias` deep inside the surface the root is bias/cos θ short of
    that, 12 Δ under max_dist: every ray is decided, blocked — measured, 0 pixels queued.)"""
    sc = _floor(tc._scene(w, h))
    sc.add_sphere((0.0, 30.0, 5.0), 2.0, RED)
    sc.add_light((0.0, 28.0, 5.0), (1.0, 1.0, 1.0), 2000.0)
    return sc


def tilted(w, h):
    """Tilted planes with normals that are not unit vectors."""
    sc = tc._scene(w, h)
    sc.add_plane((0.0, -10.0, 0.0), (0.1, 1.7, -0.2), GREY)
    sc.add_plane((0.0, 0.0, 15.0), (0.2, 0.1, -1.5), BLUE)
    sc.add_sphere((-3.0, -5.0, 6.0), 1.5, RED)
    sc.add_sphere((4.0, -7.5, 2.0), 1.0, RED)
    sc.add_light((3.0, 11.0, -6.0), (1.0, 1.0, 1.0), 400.0)
    return sc


SCENES = {"one_sphere": one_sphere, "wall_line": wall_line, "sixteen": sixteen,
          "four_lights": four_lights, "light_behind_camera": light_behind_camera,
          "small_sphere": small_sphere, "light_in_sphere": light_in_sphere, "tilted": tilted}
MOVED = [(0.7, -0.4, -22.5), (-3.0, 2.0, -27.0)]


@functools.lru_cache(maxsize=None)
def _reference(kind, size, pos, bias):
    """The oracle's frame and its Reinhard bytes, computed once and shared (read-only)."""
    from oracle import pyoracle
    sc = SCENES[kind](*size)
    sc = dataclasses.replace(sc, camera=dataclasses.replace(sc.camera, position=tuple(pos)))
    ref, _, _ = pyoracle.render(sc, max_recursion=10, bias=bias)
    ref8 = pyoracle.tonemap(ref, 1).reshape(size[1], size[0], 3)
    ref.setflags(write=False)
    ref8.setflags(write=False)
    return ref, ref8


def _delta(now, before):
    return tuple(int(v) for v in np.array(now) - before)


def _check(ctx, monkeypatch, kind, size, plan=None, bias=BIAS, moving=False, fixup=False):
    """`moving`: a batch of three different cameras (three tables, three lists of different
    lengths); otherwise the scene's camera three times.  `fixup`: the split launch must queue
    pixels for the fix-up launch, the same number under every switch."""
    plan = plan or {}
    w, h = size
    sc = SCENES[kind](w, h)
    rows = tc._plan_rows(h, plan)
    pos = [tuple(sc.camera.position)] + (MOVED if moving else [])
    cams = pos if moving else pos * 3
    refs = [_reference(kind, size, p, bias) for p in pos]
    monkeypatch.setenv("RTAMD_PK_FIX", "1")
    outs, queued = {}, {}
    for sw in SWITCHES:
        for name, v in zip(("RTAMD_PK_TILE_SHADOWED", "RTAMD_PK_TILE_SPLIT",
                            "RTAMD_PK_PLANE_CLEAR"), sw):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, v)
        split_on, shadowed_on = sw[1] is None, sw[0] is None and sw[1] is None
        ds = ctx.scene(sc)
        try:
            opts = capi.default_opts(tonemap=1, bias=bias, flags=capi.RT_FLAG_NO_TILE_ORDER,
                                     **plan)
            for rnd in range(3):
                split0 = np.array(ctx.debug_tile_split())
                sh0 = np.array(ctx.debug_tile_shadowed())
                got, got8 = tc._batch(ctx, ds, ds.cameras(np.array(cams, np.float64)), opts,
                                      len(rows), w)
                third = rnd == 2
                assert _delta(ctx.debug_tile_split(), split0) == \
                    ((3, 0) if third and split_on else (0, 3)), (sw, rnd)
                # (3, 0): a launch over the batch's shadowed lists, so the scene has such tiles
                assert _delta(ctx.debug_tile_shadowed(), sh0) == \
                    ((3, 0) if third and shadowed_on else (0, 3)), (sw, rnd)
                for f, p in enumerate(cams):
                    ref, ref8 = refs[pos.index(p)]
                    assert np.array_equal(got[f], ref[rows]), (sw, rnd, f)
                    assert np.array_equal(got[f].astype(np.float32),
                                          ref[rows].astype(np.float32)), (sw, rnd, f)
                    assert np.array_equal(got8[f], ref8[rows]), (sw, rnd, f)
            outs[sw] = (got, got8)
            queued[sw] = ctx.debug_fixup_count()
        finally:
            ds.close()
    first = outs[SWITCHES[0]]
    for sw in SWITCHES[1:]:  # identical arrays across the switches
        assert np.array_equal(outs[sw][0], first[0]) and np.array_equal(outs[sw][1], first[1]), sw
    assert len(set(queued.values())) == 1, queued
    if fixup:
        assert queued[SWITCHES[0]] > 0, queued


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", sorted(SCENES))
def test_shadowed_tiles_are_the_oracles(ctx, monkeypatch, kind, size):
    _check(ctx, monkeypatch, kind, size, fixup=kind == "light_in_sphere")


@pytest.mark.parametrize("kind", ["wall_line", "light_in_sphere"])
def test_a_row_plan_is_the_oracles_rows(ctx, monkeypatch, kind):
    _check(ctx, monkeypatch, kind, (100, 60), plan=tc.PLANS["8x2"],
           fixup=kind == "light_in_sphere")


@pytest.mark.parametrize("bias", [0.9, 1e-6])
@pytest.mark.parametrize("size", SIZES[:2], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_large_and_a_small_bias(ctx, monkeypatch, bias, size):
    """(0.9: under 1, directLightning drops a light whose transmittance is <= bias)"""
    _check(ctx, monkeypatch, "wall_line", size, bias=bias)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_three_cameras_with_different_lists(ctx, monkeypatch, size):
    _check(ctx, monkeypatch, "four_lights", size, moving=True)
