"""The shadow-plane keep masks (shadow_plane_keep in csrc/rt_shadow_table.hpp, formed by
packet_cone_table_kernel into the class words' bits 8 and up): pk_uniform_tile leaves a plane its
tile's mask drops out of the shadow classification of that light.  A dropped plane never sets
`blocked` or `undecided`, so frames are the same bits either way: every frame here is rendered
under RTAMD_PK_PLANE_CLEAR x RTAMD_PK_TILE_CLASS x RTAMD_PK_FIX in {0, 1} — as a batch of two
camera positions (ring tables), as a batch of one cached position and as one-frame launches of a
cached camera — and its HDR and Reinhard bytes are compared bit for bit with the C oracle;
rt_debug_plane_clear shows which frames were enqueued with masks.

The scenes put the rule's cases in front of the kernel:
    front          floor and wall, the light in front of both: every mask of a plane tile is 0
    behind_wall    the light behind the wall: the wall blocks the floor's shadow rays, so the
                   floor tiles' masks must keep it (dropping it would light the floor)
    on_plane       a light within 2 bias of the floor and one exactly on the wall: neither margin
                   holds, the planes stay, undecided pixels still reach the fix-up
    below_floor    the camera below the floor: the shading normals flip
    tilted         a tilted pair of planes with normals of length 0.6 and 0.8
    three_lights   in front, behind the wall and below the floor: three differing masks per tile
    big_bias       bias 0.9: every ball grows by it and a light must clear the planes by twice it
    small_bias     bias 1e-6, under 1e-7 of the scene's coordinates: the own-plane condition fails
                   and every tile keeps its own plane
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
CAM = (0.0, 0.0, -25.0)
SECOND = (0.7, -0.4, -22.5)
BIAS = 1e-3
GREY, BLUE, RED = Material((0.9, 0.9, 0.9)), Material((0.7, 0.8, 0.9)), Material((0.9, 0.3, 0.2))
# (RTAMD_PK_PLANE_CLEAR, RTAMD_PK_TILE_CLASS, RTAMD_PK_FIX)
SWITCHES = [(c, t, f) for c in "10" for t in "10" for f in "10"]


def _scene(w, h, cam=CAM):
    return SceneData(Camera(cam, w / 2.0, w, h, 0.0, 200.0, 1), name="plane_clear")


def _floor_wall(sc):
    sc.add_plane((0.0, -10.0, 0.0), (0.0, 1.0, 0.0), GREY)
    sc.add_plane((0.0, 0.0, 15.0), (0.0, 0.0, -1.0), BLUE)
    return sc


def _spheres(sc):
    sc.add_sphere((-4.0, -8.5, 4.0), 1.5, RED)
    sc.add_sphere((5.0, -4.0, 9.0), 1.0, RED)
    return sc


def front(w, h):
    sc = _spheres(_floor_wall(_scene(w, h)))
    sc.add_light((3.0, 11.0, -12.0), (1.0, 1.0, 1.0), 300.0)
    return sc


def behind_wall(w, h):
    sc = _spheres(_floor_wall(_scene(w, h)))
    sc.add_light((0.0, 5.0, 25.0), (1.0, 1.0, 1.0), 300.0)
    return sc


def on_plane(w, h):
    sc = _spheres(_floor_wall(_scene(w, h)))
    sc.add_light((6.0, -10.0 + 1.5 * BIAS, -3.0), (1.0, 1.0, 1.0), 60.0)
    sc.add_light((-6.0, 3.0, 15.0), (1.0, 0.9, 0.8), 60.0)
    return sc


def below_floor(w, h):
    sc = _floor_wall(_scene(w, h, cam=(1.0, -22.0, -25.0)))
    sc.add_sphere((0.0, -13.0, 0.0), 1.5, RED)
    sc.add_sphere((-5.0, -11.0, 6.0), 1.0, RED)
    sc.add_light((2.0, -30.0, -5.0), (1.0, 1.0, 1.0), 300.0)
    sc.add_light((2.0, 8.0, -5.0), (1.0, 1.0, 1.0), 300.0)
    return sc


def tilted(w, h):
    sc = _scene(w, h)
    sc.add_plane((0.0, -10.0, 0.0), (0.06, 0.594, -0.06), GREY)     # |n| = 0.6
    sc.add_plane((0.0, 0.0, 15.0), (0.16, -0.08, -0.78), BLUE)      # |n| = 0.8
    _spheres(sc)
    sc.add_light((3.0, 11.0, -12.0), (1.0, 1.0, 1.0), 300.0)
    sc.add_light((-8.0, 2.0, 30.0), (1.0, 1.0, 1.0), 300.0)
    return sc


def three_lights(w, h):
    sc = _spheres(_floor_wall(_scene(w, h)))
    sc.add_light((3.0, 11.0, -12.0), (1.0, 1.0, 1.0), 150.0)
    sc.add_light((0.0, 5.0, 25.0), (1.0, 0.8, 0.8), 200.0)
    sc.add_light((-2.0, -16.0, 3.0), (0.8, 0.8, 1.0), 200.0)
    return sc


SCENES = {"front": front, "behind_wall": behind_wall, "on_plane": on_plane,
          "below_floor": below_floor, "tilted": tilted, "three_lights": three_lights,
          "big_bias": front, "small_bias": front}
BIASES = {"big_bias": 0.9, "small_bias": 1e-6}  # (0.9 < 1: a light with T <= bias is dropped)


@functools.lru_cache(maxsize=None)
def _reference(kind, size, pos):
    """The oracle's frame and Reinhard bytes, computed once per frame and shared (read-only)."""
    from oracle import pyoracle
    sc = SCENES[kind](*size)
    sc = dataclasses.replace(sc, camera=dataclasses.replace(sc.camera, position=tuple(pos)))
    ref, _, _ = pyoracle.render(sc, max_recursion=10, bias=BIASES.get(kind, BIAS))
    ref8 = pyoracle.tonemap(ref, 1).reshape(size[1], size[0], 3)
    ref.setflags(write=False)
    ref8.setflags(write=False)
    return ref, ref8


def _plan_rows(h, plan):
    o = capi.default_opts(**plan)
    if o.row_cycle <= 1 or o.row_block == 0:
        return list(range(o.row_begin, h))
    rows = []
    for b in range(o.row_begin, h, o.row_block * o.row_cycle):
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
    return tuple(np.array(ctx.debug_plane_clear()) - before)


def _check_all_switches(ctx, monkeypatch, kind, size, plan=None):
    plan = plan or {}
    w, h = size
    sc = SCENES[kind](w, h)
    bias = BIASES.get(kind, BIAS)
    rows = _plan_rows(h, plan)
    pos = [tuple(sc.camera.position), SECOND]
    refs = [_reference(kind, size, p) for p in pos]
    for clear, cls, fix in SWITCHES:
        monkeypatch.setenv("RTAMD_PK_PLANE_CLEAR", clear)
        monkeypatch.setenv("RTAMD_PK_TILE_CLASS", cls)
        monkeypatch.setenv("RTAMD_PK_FIX", fix)
        # masks ride in the class words: formed only where those are, and only with the switch on
        want = (lambda n: (n, 0)) if clear == "1" and cls == "1" else (lambda n: (0, n))
        tag = (kind, size, clear, cls, fix)
        ds = ctx.scene(sc)
        try:
            # (no tile order: a launch that records wave durations takes the general variant)
            opts = capi.default_opts(tonemap=1, bias=bias, flags=capi.RT_FLAG_NO_TILE_ORDER,
                                     **plan)
            assert capi.rendered_rows(opts, h) == len(rows)
            for cams in (pos, [pos[0], pos[0]]):
                before = np.array(ctx.debug_plane_clear())
                got, got8 = _batch(ctx, ds, ds.cameras(np.array(cams, np.float64)), opts,
                                   len(rows), w)
                assert _used(ctx, before) == want(2), (tag, cams)
                for f, p in enumerate(cams):
                    ref, ref8 = refs[pos.index(p)]
                    assert np.array_equal(got[f], ref[rows]), (tag, cams, f)
                    assert np.array_equal(got8[f], ref8[rows]), (tag, cams, f)
            for k in range(3):  # one-frame launches, the camera cached by now
                before = np.array(ctx.debug_plane_clear())
                out = ds.render(hdr64=True, tonemap=1, opts=opts)
                if k == 2:
                    assert _used(ctx, before) == want(1), tag
                assert np.array_equal(out["hdr64"], refs[0][0][rows]), (tag, k)
                assert np.array_equal(out["ldr"], refs[0][1][rows]), (tag, k)
        finally:
            ds.close()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", sorted(SCENES))
def test_scene_kinds_are_the_oracles(ctx, monkeypatch, kind, size):
    _check_all_switches(ctx, monkeypatch, kind, size)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_row_plan_is_the_oracles_rows(ctx, monkeypatch, size):
    _check_all_switches(ctx, monkeypatch, "three_lights", size,
                        plan=dict(row_block=3, row_cycle=3))


def test_behind_wall_floor_is_dark():
    """The scene does what its name says (the oracle's frame, no GPU): with the light behind the
    wall the floor's bottom row receives nothing, so a mask that dropped the wall would show."""
    ref, _ = _reference("behind_wall", (64, 40), CAM)
    lit, _ = _reference("front", (64, 40), CAM)
    assert np.all(ref[-1] == 0.0) and np.all(lit[-1].max(axis=-1) > 0.0)
