"""GPU parity of the packet kernel's wave-uniform shortcuts, bit for bit against the C oracle.

packet_direct_kernel (rt_packet_kernel.hpp), in its variants for scenes of up to 64 spheres, reads the
camera ray's frame constants (W/2, H/2, dz = (cam.z + focal) - cam.z, dz*dz) from the host
(camera_consts) and sends a wave whose sphere mask is empty straight to the planes, for camera
rays and for shadow rays.  None of it may change a bit: every frame here is compared with the
oracle through both C2 variants — the fix-up variant (RTAMD_PK_FIX=1, a batch) and the marching
variant (RTAMD_PK_FIX=0).  The plane scenes at the end pin the shadow classification of the
plane a packet stands on (a skip of that plane was measured and not kept: DESIGN §4).
"""
import dataclasses

import numpy as np
import pytest
import torch

from raytracingengine_amd import capi
from raytracingengine_amd.scene import Camera, Material, SceneData

pytestmark = pytest.mark.gpu

VARIANTS = ["fixup", "march"]


def _moved(sc, pos):
    return dataclasses.replace(sc, camera=dataclasses.replace(sc.camera, position=tuple(pos)))


def _batch(ctx, ds, sc, positions, opts):
    """rt_render_batch of one frame per camera position: [(hdr[rows, W, 3], ldr[rows, W, 3])]."""
    w, h = sc.camera.width, sc.camera.height
    rows, n = capi.rendered_rows(opts, h), len(positions)
    H64 = torch.full((n * rows * w * 3,), -1.0, dtype=torch.float64, device="cuda")
    L8 = torch.zeros(n * rows * w * 3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ds.render_batch(ds.cameras(np.asarray(positions, np.float64)), H64.data_ptr(), None,
                    L8.data_ptr(), opts)
    ctx.synchronize()
    return list(zip(H64.cpu().numpy().reshape(n, rows, w, 3),
                    L8.cpu().numpy().reshape(n, rows, w, 3)))


def _frames(ctx, sc, variant, monkeypatch, bias=1e-3):
    """The scene's frame through one variant: a batch of 2 (fix-up) or a single launch."""
    monkeypatch.setenv("RTAMD_PK_FIX", "1" if variant == "fixup" else "0")
    ds = ctx.scene(sc)
    try:
        if variant == "fixup":
            return _batch(ctx, ds, sc, [sc.camera.position] * 2,
                          capi.default_opts(tonemap=1, bias=bias))
        out = ds.render(hdr64=True, tonemap=1, bias=bias)
        return [(out["hdr64"], out["ldr"])]
    finally:
        ds.close()


def _assert_equal(frames, ref, ref8):
    for hdr, ldr in frames:
        assert np.array_equal(hdr.view(np.int64), ref.view(np.int64)), \
            np.argwhere(hdr.view(np.int64) != ref.view(np.int64))[:8]
        assert np.array_equal(ldr, ref8)


# ------------------------------------------------------------------ frame constants
# Cameras on both sides of 2^27, where the spacing of doubles changes: (z + 0.7) - z is not 0.7
# and differs from camera to camera
Z0 = 2.0 ** 27 - 0.2
FOCAL = 0.7
SIZES = [(1, 1), (8, 8), (9, 7), (193, 109)]  # odd sizes: W/2 and H/2 are not integers
CAMS = [(0.0, 0.0, Z0), (0.25, -0.125, Z0 + 0.1), (-1.5, 0.5, Z0 - 0.5), (0.1, 0.2, Z0 + 0.4),
        (3.0, 1.0, Z0 + 0.25)]


def _const_scene(w, h):
    sc = SceneData(Camera(CAMS[0], FOCAL, w, h, 0.0, 200.0, 1), name=f"consts_{w}x{h}")
    sc.add_sphere((0.0, 0.0, Z0 + 5.0), 4.5, Material((0.8, 0.4, 0.3)))
    sc.add_plane((0.0, -3.0, 0.0), (0.0, 1.0, 0.0), Material((0.7, 0.8, 0.9)))
    sc.add_plane((0.0, 0.0, Z0 + 15.0), (0.0, 0.0, -1.0), Material((0.5, 0.9, 0.6)))
    sc.add_light((3.0, 6.0, Z0 - 1.0), (1.0, 1.0, 1.0), 60.0)
    return sc


@pytest.fixture(scope="module")
def const_refs(oracle):
    """{(w, h): [(oracle HDR, Reinhard bytes) per camera of CAMS]}, rendered once."""
    out = {}
    for w, h in SIZES:
        sc = _const_scene(w, h)
        refs = []
        for pos in CAMS:
            ref, _, _ = oracle.render(_moved(sc, pos))
            refs.append((ref, oracle.tonemap(ref, 1).reshape(ref.shape)))
        out[w, h] = refs
    return out


def test_dz_is_not_the_focal_length():
    for pos in CAMS:
        z = np.float64(pos[2])
        assert (z + np.float64(FOCAL)) - z != np.float64(FOCAL)
    assert len({(np.float64(p[2]) + np.float64(FOCAL)) - np.float64(p[2]) for p in CAMS}) > 1


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frame_constants_vs_oracle(ctx, const_refs, monkeypatch, size, variant):
    """Five cameras in one rt_render_batch (each frame reads its own record), the same batch
    over a block-cyclic row set, and a single launch per camera (TraceParams' own constants)."""
    w, h = size
    sc = _const_scene(w, h)
    refs = const_refs[size]
    monkeypatch.setenv("RTAMD_PK_FIX", "1" if variant == "fixup" else "0")
    ds = ctx.scene(sc)
    try:
        for (hdr, ldr), (ref, ref8) in zip(
                _batch(ctx, ds, sc, CAMS, capi.default_opts(tonemap=1)), refs):
            _assert_equal([(hdr, ldr)], ref, ref8)
        r0 = 1 if h > 1 else 0
        opts = capi.default_opts(tonemap=1, row_begin=r0, row_block=2, row_cycle=2)
        rows = [y for b in range(r0, h, 4) for y in range(b, min(b + 2, h))]
        assert len(rows) == capi.rendered_rows(opts, h)
        for (hdr, ldr), (ref, ref8) in zip(_batch(ctx, ds, sc, CAMS, opts), refs):
            _assert_equal([(hdr, ldr)], ref[rows], ref8[rows])
    finally:
        ds.close()
    for pos, (ref, ref8) in list(zip(CAMS, refs))[:2]:
        moved = _moved(sc, pos)
        ds = ctx.scene(moved)
        try:
            out = ds.render(hdr64=True, tonemap=1)
        finally:
            ds.close()
        _assert_equal([(out["hdr64"], out["ldr"])], ref, ref8)


# ------------------------------------------------------------------ empty masks, planes underfoot
W, H = 64, 40
GREY, BLUE = Material((0.9, 0.9, 0.9)), Material((0.7, 0.8, 0.9))


def _room(cam=(0.0, 0.0, -10.0), focal=40.0, wall=True, floor_n=(0.0, 1.0, 0.0), name="room"):
    sc = SceneData(Camera(cam, focal, W, H, 0.0, 200.0, 1), name=name)
    sc.add_plane((0.0, -3.0, 0.0), floor_n, GREY)
    if wall:
        sc.add_plane((0.0, 0.0, 12.0), (0.0, 0.0, -1.0), BLUE)
    return sc


def _no_spheres():
    sc = _room(name="no_spheres")
    sc.add_light((2.0, 5.0, -2.0), (1.0, 1.0, 1.0), 60.0)
    return sc


def _behind():  # 16 spheres, all behind the camera: every cone mask is empty
    sc = _no_spheres()
    for i in range(16):
        sc.add_sphere((i % 4 * 2.0 - 3.0, i // 4 * 2.0 - 3.0, -16.0 - i), 0.8,
                      Material((0.8, 0.3 + 0.03 * i, 0.4)))
    return sc


def _unoccluding():  # visible spheres above a light that hangs below them: nothing is shadowed
    sc = _room(wall=False, name="unoccluding")
    for i in range(4):
        sc.add_sphere((-3.75 + 2.5 * i, 2.5, 4.0), 1.0, Material((0.3, 0.7, 0.2 + 0.1 * i)))
    sc.add_light((0.0, -1.0, 0.0), (1.0, 1.0, 1.0), 40.0)
    return sc


def _touching():  # tests/test_gpu_batch.py's undecided-shadow arrangement at this size
    sc = SceneData(Camera((0.0, 0.0, -25.0), 32.0, W, H, 0.0, 200.0, 1), name="touching")
    for i in range(8):
        sc.add_sphere((-7.0 + 2.0 * i, -9.0, 3.0), 1.0, Material((0.8, 0.3 + 0.05 * i, 0.4)))
        sc.add_sphere((-7.0 + 2.0 * i, -7.0, 3.0), 1.0, Material((0.3, 0.7, 0.2 + 0.05 * i)))
    sc.add_plane((0.0, -10.0, 0.0), (0.0, 1.0, 0.0), GREY)
    sc.add_plane((0.0, 0.0, 15.0), (0.0, 0.0, -1.0), BLUE)
    sc.add_light((0.3, -5.9, 3.0), (1.0, 1.0, 1.0), 40.0)
    return sc


def _grazing():  # n·L = 3e-5 / dist over the floor: on both sides of Plane::Intersect's 1e-6
    sc = _room(wall=False, name="grazing")
    sc.add_light((0.0, -3.0 + 3e-5, 10.0), (1.0, 1.0, 1.0), 50.0)
    sc.add_light((4.0, 6.0, 0.0), (0.2, 0.2, 0.2), 30.0)
    return sc


def _in_plane():  # a light exactly in the floor's plane, one a hair behind it
    sc = _room(name="in_plane")
    sc.add_light((0.0, -3.0, 10.0), (1.0, 1.0, 1.0), 50.0)
    sc.add_light((5.0, -3.0 - 1e-9, 8.0), (1.0, 0.5, 0.5), 50.0)
    sc.add_light((-2.0, 5.0, -2.0), (0.3, 0.3, 0.3), 40.0)
    return sc


def _far_floor():  # a camera 1e6 above the floor: every hit at t ~ 1e6
    sc = _room(cam=(0.0, 1e6, -10.0), wall=False, name="far_floor")
    sc.add_sphere((10.0, -2.0, 30.0), 1.0, Material((0.8, 0.4, 0.3)))
    sc.add_light((0.0, 50.0, 20.0), (1.0, 1.0, 1.0), 1e4)
    return sc


def _non_unit():  # stored normals of length 1.5 (|n|_1 <= 2: prologue normal) and 3 (> 2: not)
    sc = SceneData(Camera((0.0, 0.0, -10.0), 40.0, W, H, 0.0, 200.0, 1), name="non_unit")
    sc.add_plane((0.0, -3.0, 0.0), (0.0, 1.5, 0.0), GREY)
    sc.add_plane((0.0, 0.0, 12.0), (0.0, 0.0, -3.0), BLUE)
    sc.add_sphere((1.0, -1.0, 4.0), 1.5, Material((0.8, 0.4, 0.3)))
    sc.add_light((2.0, 5.0, -2.0), (1.0, 1.0, 1.0), 60.0)
    return sc


def _back():  # the floor stored with its normal pointing down: seen from its back
    sc = _room(floor_n=(0.0, -1.0, 0.0), name="back")
    sc.add_sphere((1.0, -1.0, 4.0), 1.5, Material((0.8, 0.4, 0.3)))
    sc.add_light((2.0, 5.0, -2.0), (1.0, 1.0, 1.0), 60.0)
    return sc


def _coincident():  # two floors in one place, and a third stored with another point and length
    sc = _room(name="coincident")
    sc.add_plane((0.0, -3.0, 0.0), (0.0, 1.0, 0.0), Material((0.2, 0.9, 0.2)))
    sc.add_plane((5.0, -3.0, 1.0), (0.0, 2.0, 0.0), Material((0.9, 0.2, 0.2)))
    sc.add_sphere((1.0, -1.0, 4.0), 1.5, Material((0.8, 0.4, 0.3)))
    sc.add_light((2.0, 5.0, -2.0), (1.0, 1.0, 1.0), 60.0)
    return sc


def _mixed():  # floor, wall and spheres in view: tiles straddle them
    sc = _room(name="mixed")
    sc.add_sphere((1.0, -1.0, 4.0), 1.5, Material((0.8, 0.4, 0.3)))
    sc.add_sphere((-3.0, -2.0, 8.0), 1.0, Material((0.3, 0.4, 0.8)))
    sc.add_light((2.0, 5.0, -2.0), (1.0, 1.0, 1.0), 60.0)
    sc.add_light((-6.0, 1.0, 2.0), (1.0, 0.8, 0.6), 30.0)
    return sc


MASK_SCENES = {"no_spheres": _no_spheres, "behind": _behind, "unoccluding": _unoccluding,
               "touching": _touching}
SELF_SCENES = {"grazing": _grazing, "in_plane": _in_plane, "far_floor": _far_floor,
               "non_unit": _non_unit, "back": _back, "coincident": _coincident, "mixed": _mixed}
BIASES = [1e-3, 1e-12]


@pytest.fixture(scope="module")
def scene_refs(oracle):
    """{(scene, bias): (scene, oracle HDR, Reinhard bytes)}, rendered once."""
    out = {}
    for name, make in {**MASK_SCENES, **SELF_SCENES}.items():
        for bias in (BIASES if name in SELF_SCENES else BIASES[:1]):
            sc = make()
            ref, _, _ = oracle.render(sc, bias=bias)
            out[name, bias] = (sc, ref, oracle.tonemap(ref, 1).reshape(ref.shape))
    return out


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(MASK_SCENES))
def test_empty_sphere_masks_vs_oracle(ctx, scene_refs, monkeypatch, name, variant):
    """No spheres at all, spheres only behind the camera (empty cone masks), spheres in view
    that shadow nothing (empty shadow masks next to occupied cone masks), and spheres resting on
    the floor around the light (occupied masks, many undecided shadow rays)."""
    sc, ref, ref8 = scene_refs[name, BIASES[0]]
    _assert_equal(_frames(ctx, sc, variant, monkeypatch), ref, ref8)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("bias", BIASES)
@pytest.mark.parametrize("name", list(SELF_SCENES))
def test_shadow_rays_from_planes_vs_oracle(ctx, scene_refs, monkeypatch, name, bias, variant):
    """Shadow rays that start on a plane, at the default bias and at 1e-12 (origins all but on
    the plane): a floor lit at grazing incidence (n.L on both sides of 1e-6), lights in and just
    behind the floor's plane, hits at t ~ 1e6, stored normals of other lengths, a plane seen from
    its back, coincident planes, and tiles that straddle floor, wall and spheres."""
    sc, ref, ref8 = scene_refs[name, bias]
    _assert_equal(_frames(ctx, sc, variant, monkeypatch, bias=bias), ref, ref8)
