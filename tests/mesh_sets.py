"""Crafted mesh scenes for the packet kernels' triangle path: the wave-coherent BVH walk (bvh_wave,
csrc/rt_packet_device.hpp), which a render of an opaque mesh scene without reflection runs for its
camera rays and for its shadow march, and which the packet G-buffer kernel runs too.  One module
for tests/test_mesh_sets.py (which checks on the CPU that every scene still has the edges it
exists for), tests/test_bvh_walk_host.py (which hands the meshes to the emulated walks of
tests/bvh_walk/walk_main.cpp) and tests/test_gpu_mesh_packet.py (which renders them).

Every material is opaque with specular 0, so rt_render takes kPathDirect and with it the packet
kernel (rt_capi.cpp enqueue_frames); the grids of tests/raysets.py give every second triangle
specular 0.3 and render on the chain path instead.  Every triangle has a colour of its own (three
components from its index modulo 5, 7 and 11, none zero: distinct for 385 indices in a row), so a
tie that goes to the wrong triangle shows in the image; the triangles' order is shuffled with a
fixed seed, so the builder does not meet the lowest index of a tie first by construction.

Camera::getRay (Math.h:99-121) computes d = unit((x - W/2, H/2 - y, pos.z + focal) - pos) in
absolute world units: a camera at integer (cx, cy) with an even image size has one column with
d.x == 0 and one row with d.y == 0, exactly.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from raysets import CELL, GRID, _bump, _grid_tris, _rng
from raytracingengine_amd.scene import Camera, Material, SceneData

SIZE = (64, 48)
BIAS = 1e-3
SPECULAR_ON = 5e-4          # a specular that is not above the bias: Blinn-Phong without reflection
LIGHT = ((4.0, 10.0, -5.0), (1.0, 1.0, 1.0), 100.0)     # raysets.grid_scene's
LIGHT_BELOW = ((3.0, -4.0, 3.0), (1.0, 0.9, 0.8), 60.0)
LIGHT_WALL = ((6.0, 2.0, 2.0), (1.0, 1.0, 1.0), 60.0)   # grazes the wall z = 4 from the camera's side
LIGHT_FAN = ((1.0, 2.0, -3.0), (1.0, 1.0, 1.0), 80.0)
FAN = 300


def tri_material(k: int) -> Material:
    return Material(((k % 5 + 1) / 6.0, (k % 7 + 1) / 8.0, (k % 11 + 1) / 12.0))


def _plain(color):
    return Material(color)


def _flat(a, b):
    return 0.0


def _stand(p):
    """A grid vertex (x, height, z), x and z in [0, 6], stood up in the plane z = 4."""
    return (p[0] - GRID * CELL / 2.0, p[2] - GRID * CELL / 2.0, 4.0 + p[1])


def _shuffled(tris, *names):
    return [tris[k] for k in _rng("mesh_sets", *names).permutation(len(tris))]


def _scene(name, pos, focal, tris, lights, size=SIZE, far=200.0, aa=1):
    sc = SceneData(Camera(tuple(map(float, pos)), float(focal), size[0], size[1], 1.0, far, aa),
                   name=f"mesh_{name}")
    for k, (v0, v1, v2) in enumerate(tris):
        sc.add_triangle(v0, v1, v2, tri_material(k))
    for l in lights:
        sc.add_light(*l)
    return sc


def _wall_tris(height, tag):
    return _shuffled([tuple(_stand(p) for p in t) for t in _grid_tris(height)], tag)


def wall(size=SIZE, lights=(LIGHT_WALL,)):
    """The flat grid in z = 4 seen head on: hit points sx/8, so every sixth column and row of
    pixels lies on a grid line (off the 8-pixel tile edges), the d.x == 0 column and the d.y == 0
    row among them; every node box has zero thickness in z."""
    return _scene("wall", (0, 0, -2), 48, _wall_tris(_flat, "wall"), lights, size)


def wall_bumpy():
    """The bumpy grid stood up the same way: the grazing light makes the bumps shadow each other,
    so the shadow march walks the BVH with part of each wave's lanes."""
    return _scene("wall_bumpy", (0, 0, -2), 48, _wall_tris(_bump, "wall_bumpy"), (LIGHT_WALL,))


def floor():
    """The flat grid in y = 0: zero-thickness boxes at coordinate 0, where the build's relative
    widening vanishes and only its 1e-300 is left."""
    return _scene("floor", (3, 3, -3), 40, _shuffled(_grid_tris(_flat), "floor"), (LIGHT,))


def inplane():
    """The camera in the mesh's own plane: nothing is hit; the slab test of the y axis sees
    t0 == t1 = ±0, and the d.y == 0 row has its origin inside the degenerate slab."""
    return _scene("inplane", (3, 0, -4), 40, _shuffled(_grid_tris(_flat), "floor"), (LIGHT,))


def inside():
    """The camera inside the bumpy grid's root box and many of its node boxes; the light below
    makes the faces seen from below cast shadow rays."""
    return _scene("inside", (3, 0.125, 1.5), 24, _shuffled(_grid_tris(_bump), "inside"),
                  (LIGHT, LIGHT_BELOW))


def behind():
    """raysets.grid_scene('behind') with plain materials: the walk starts with a sphere's or a
    plane's hit to beat (one plane lies in the grid itself) and wins only when strictly closer."""
    sc = _scene("behind", (3, 3, -3), 40, _shuffled(_grid_tris(_flat), "floor"), (LIGHT,))
    sc.add_sphere((3.0, 1.5, 3.0), 1.0, _plain((0.9, 0.4, 0.2)))
    sc.add_plane((0.0, 0.5, 0.0), (0.0, 1.0, 0.125), _plain((0.7, 0.8, 0.9)))
    sc.add_plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), _plain((0.9, 0.9, 0.9)))
    return sc


def canopy(upper=True):
    """floor plus a half-size flat grid at y = 1.5 over its middle: the floor's shadow rays meet
    flat nodes from below."""
    tris = _shuffled(_grid_tris(_flat), "floor")
    if upper:
        up = [tuple((1.5 + 0.5 * p[0], 1.5, 1.5 + 0.5 * p[2]) for p in t)
              for t in _grid_tris(_flat)]
        tris = tris + _shuffled(up, "canopy")
    return _scene("canopy" if upper else "canopy_floor", (3, 4, -3), 40, tris,
                  (LIGHT, ((1.0, 8.0, 4.0), (0.9, 1.0, 0.8), 60.0)))


def far(bumpy=False):
    """The walls from 2^27 away through a focal length of 2^30: t is about 1.3e8, so the absolute
    rounding of a slab parameter (1.5e-8) exceeds the boxes' 1e-9 relative widening (4e-9), and
    only the walk's own relative margins keep it conservative."""
    tris = _wall_tris(_bump, "wall_bumpy") if bumpy else _wall_tris(_flat, "wall")
    return _scene("far_bumpy" if bumpy else "far", (0, 0, -(2.0 ** 27)), 2.0 ** 30, tris,
                  (LIGHT_WALL,), far=1e12)


def _fan_tris():
    tris = []
    for k in range(FAN):
        y0 = (k % 7) / 8.0 - 1.0
        tris.append(((0.0, y0, 4.0), (2.0 ** -k, y0, 4.0), (0.0, y0 + 1.0, 4.0)))
    return _shuffled(tris, "fan")


def fan(focal=2.0 ** 14):
    """300 coplanar slivers along x = 0 whose widths halve: the builder takes them to its depth
    cap (48) with a leaf of 60 at the cap, the d.x == 0 column has its origin on the face x = 0
    of every nested box, and at focal 2^14 every hit is a many-way exact tie."""
    return _scene("fan", (0, 0, -2), focal, _fan_tris(), (LIGHT_FAN,))


FAN_SPHERES = 70    # two chunks of 64: the packet kernel's MAXC = 4 instantiation (rt_packet.hip)


def fan_spheres():
    """fan with 70 small spheres on a fixed lattice beside it, the first two moved behind it: one
    behind its empty half (seen), one behind its covered half (hidden)."""
    sc = fan()
    sc.name = "mesh_fan_spheres"
    for i in range(FAN_SPHERES):
        c = (0.75 + 0.5 * (i % 7), -2.0 + 0.5 * (i // 7 % 5), 3.0 + 1.5 * (i // 35))
        if i == 0:
            c, r = (-0.0078125, 0.001953125, 6.0), 0.00390625
        elif i == 1:
            c, r = (0.0078125, -0.001953125, 6.0), 0.00390625
        else:
            r = 0.125
        sc.add_sphere(c, r, _plain(((i % 3 + 1) / 4.0, (i % 4 + 1) / 5.0, (i % 5 + 1) / 6.0)))
    return sc


SCENES = {
    "wall": wall,
    "wall_60x44": lambda: wall((60, 44)),
    "floor": floor,
    "inplane": inplane,
    "wall_bumpy": wall_bumpy,
    "inside": inside,
    "behind": behind,
    "canopy": canopy,
    "far": far,
    "far_bumpy": lambda: far(True),
    "fan_f48": lambda: fan(48.0),
    "fan": fan,
    "fan_spheres": fan_spheres,
    "wall_nolight": lambda: wall(lights=()),
}
# the scenes the depth-cap tree is in: on the GPU only after tests/test_bvh_walk_host.py's depth
# mode has passed (the tree's depth and every walk's stack use, against kBvhStack and kPkStack)
DEPTH_CAP = ("fan_f48", "fan", "fan_spheres")
VARIANT_SCENES = ("wall", "wall_bumpy", "fan")


def with_aa(sc: SceneData, aa: int) -> SceneData:
    return dataclasses.replace(sc, camera=dataclasses.replace(sc.camera, antiAliasingAmount=aa))


def with_specular(sc: SceneData, k: int = 5) -> SceneData:
    """Triangle k's material with specular 5e-4 and shininess 24: not above the bias, so the path
    stays direct, and above 0, so Blinn-Phong is compiled in (kFeatAll)."""
    tris = list(sc.triangles)
    tris[k] = tris[k][:4] + (dataclasses.replace(tris[k][4], specular=SPECULAR_ON, shininess=24.0),)
    return dataclasses.replace(sc, triangles=tris)


def moved(sc: SceneData, pos) -> SceneData:
    return dataclasses.replace(sc, camera=dataclasses.replace(sc.camera,
                                                              position=tuple(map(float, pos))))


# ------------------------------------------------------------------ what the CPU knows of a scene
def camera_rays(sc: SceneData) -> np.ndarray:
    """The oracle's Camera::getRay of every pixel, row-major, [H*W, 6]."""
    from oracle import pyoracle as po
    L, cam = po.lib(), sc.camera.to_struct()
    rays = np.empty((sc.camera.height * sc.camera.width, 6), np.float64)
    for y in range(sc.camera.height):
        for x in range(sc.camera.width):
            L.oracle_get_ray(cam.ctypes.data, x, y, 0, 0, 0,
                             rays[y * sc.camera.width + x].ctypes.data)
    return rays


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def triangle_ts(sc: SceneData, rays: np.ndarray) -> np.ndarray:
    """Triangle::Intersect (Shape.h:202-220) of every ray with every triangle, in the reference's
    operation order (one IEEE operation per numpy call, nothing fused): [rays, triangles] of t,
    +inf where the triangle does not accept."""
    tr = sc.triangle_array()
    a0 = tr["v0"] + tr["translation"]
    e1 = (tr["v1"] + tr["translation"]) - a0
    e2 = (tr["v2"] + tr["translation"]) - a0
    col = lambda m, rowwise: [m[:, k][:, None] if rowwise else m[:, k][None, :]  # noqa: E731
                              for k in range(3)]
    o, d = col(rays[:, :3], True), col(rays[:, 3:], True)
    a0, e1, e2 = col(a0, False), col(e1, False), col(e2, False)
    with np.errstate(all="ignore"):
        h = _cross(d, e2)
        a = _dot(e1, h)
        ok = ~((a > -1e-6) & (a < 1e-6))
        f = 1.0 / a
        s = tuple(o[k] - a0[k] for k in range(3))
        u = f * _dot(s, h)
        ok &= ~((u < 0.0) | (u > 1.0))
        q = _cross(s, e1)
        v = f * _dot(d, q)
        ok &= ~((v < 0.0) | (u + v > 1.0))
        t = f * _dot(e2, q)
        ok &= t > 1e-6
    return np.where(ok, t, np.inf)


def facts(sc: SceneData) -> dict:
    """The properties a scene exists for, from the oracle and triangle_ts."""
    from oracle import pyoracle as po
    W, H = sc.camera.width, sc.camera.height
    rays = camera_rays(sc)
    ts = triangle_ts(sc, rays)
    tmin = ts.min(axis=1)
    hit = np.isfinite(tmin)
    tied = (ts == tmin[:, None]) & hit[:, None]
    ties = tied.sum(axis=1) >= 2
    lowest = np.where(hit, tied.argmax(axis=1), -1)   # the lowest index among the smallest t
    closest = po.closest_rays(sc, rays)
    img, ntrace, nshadow = po.render(sc)
    win = closest[:, 0] == 3
    ty, tx = -(-H // 8), -(-W // 8)
    partial = 0
    h2 = hit.reshape(H, W)
    for j in range(ty):
        for i in range(tx):
            blk = h2[8 * j:8 * j + 8, 8 * i:8 * i + 8]
            partial += bool(blk.any() and not blk.all())
    dark = hit & ~img.reshape(-1, 3).any(axis=1)     # a triangle on the ray, a black pixel
    return dict(rays=rays, ts=ts, hit=hit, ties=ties, lowest=lowest, closest=closest, image=img,
                trace_rays=ntrace, shadow_rays=nshadow, hits=int(hit.sum()),
                n_ties=int(ties.sum()), wins=int(win.sum()), partial_tiles=partial,
                dx0=int((rays[:, 3] == 0.0).sum()), dy0=int((rays[:, 4] == 0.0).sum()),
                dark=int(dark.sum()))


def hex_scene(sc: SceneData) -> str:
    """The scene as tests/bvh_walk/walk_main.cpp reads it, every double in hex: the triangle
    count, the image size, the camera's position and focal length and the light count; then per
    triangle v0, v1, v2 and the translation; then the lights' positions."""
    def hexes(vals):
        return " ".join(float(v).hex() for v in vals)

    tr, cam = sc.triangle_array(), sc.camera
    lines = [f"{len(tr)} {cam.width} {cam.height} {hexes((*cam.position, cam.focal))} "
             f"{len(sc.lights)}"]
    lines += [hexes(x for k in ("v0", "v1", "v2", "translation") for x in t[k]) for t in tr]
    lines += [hexes(l[0]) for l in sc.lights]
    return "\n".join(lines) + "\n"
