"""Expected answers and distance lists for the transmittance queries (rt_transmittance_rays,
Scene::computeTransmittance, Scene.h:35-77; rt_light_transmittance, the shadow rays of
Scene::directLightning, Scene.h:86-104), shared by tests/test_oracle_transmittance.py (which
checks them on the CPU) and tests/test_gpu_transmittance.py (which runs them on the device).

Every expected value is one call of the oracle's computeTransmittance (oracle_transmittance,
oracle/rt_oracle.h) for one ray and one maxDist.  The distances of a ray lie around the march's
own thresholds: the ray is marched on the CPU with the oracle's closest hit (oracle_closest) for
up to three counted hits, and each `traveled + t` — the value the march compares with maxDist —
is asked one unit in the last place below, exactly, one above, at x·(1 + 1e-9) and at 2·x.

The rays and scenes are those of tests/raysets.py.  Tables are cached per set: a reference is
computed once and left unchanged.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np

import occlusion_sets
import raysets
from raytracingengine_amd.configs import make_config
from raytracingengine_amd.scene import Material, SceneData

BIAS = raysets.BIAS
MESH_RAYS = 256   # scenes of thousands of triangles: the table covers the first MESH_RAYS rays
MESH_TRIS = 1024
COUNTED = 3       # thresholds per ray: the first COUNTED counted hits of the march
DBL_MAX = float(np.finfo(np.float64).max)
NONFINITE_SCENES = ("c2", "mesh", "glass_tri_area")
LIGHT_SCENES = ("c2", "c3", "c4", "glass", "glass_tri_area", "mesh", "bigmesh")
BVH_SCENES = ("mesh", "bigmesh")
BVH_GRIDS = ("grid_flat", "grid_bumpy", "grid_behind")
OPAQUE_SCENES = ("c2", "sph300", "c1", "mesh")   # no transparent material: the fast path's scenes


# ------------------------------------------------------------------ the oracle, one scene view
class Oracle:
    """The oracle's closest hit and computeTransmittance over one scene (its C view is built
    once and kept alive here)."""

    def __init__(self, sc: SceneData):
        from oracle import pyoracle as po
        self.lib = po.lib()
        self.view = po.OracleScene(sc)
        self.addr = ctypes.addressof(self.view.c)
        self._out = np.zeros(7, np.float64)
        self._idx = ctypes.c_int32(-1)

    def closest_t(self, ray):
        """The closest hit's t, or None on a miss."""
        r = np.ascontiguousarray(ray, np.float64)
        typ = self.lib.oracle_closest(self.addr, r.ctypes.data, self._out.ctypes.data,
                                      ctypes.byref(self._idx))
        return float(self._out[0]) if typ else None

    def transmittance(self, ray, max_dist: float, bias: float) -> float:
        r = np.ascontiguousarray(ray, np.float64)
        return self.lib.oracle_transmittance(self.addr, r.ctypes.data, float(max_dist), float(bias))


def thresholds(orc: Oracle, ray, bias: float) -> list:
    """The `traveled + t` of the march's first COUNTED counted hits, walked as the march walks:
    a hit at t <= 0 moves the origin by bias, one at t <= bias by t + bias, neither counted;
    origins advance as (o + d·t) + d·bias, in that order."""
    o = np.array(ray[:3], np.float64)
    d = np.array(ray[3:], np.float64)
    traveled, out = 0.0, []
    with np.errstate(all="ignore"):
        for _ in range(64):
            t = orc.closest_t(np.concatenate([o, d]))
            if t is None:
                break
            if t <= 0.0:
                o = o + d * bias
                traveled += bias
                continue
            if not t <= bias:
                out.append(traveled + t)
                if len(out) == COUNTED:
                    break
            o = (o + d * t) + d * bias
            traveled += t + bias
    return out


def distances(xs, bias: float, extra=()) -> list:
    """The maxDist values one ray is asked with: those that answer 1.0 whatever the scene holds
    (0, -1, NaN) or nearly so (the smallest denormal, distances within the bias steps), +inf and
    the largest finite double (the whole march), and around each threshold x one unit in the last
    place below it, x itself (`traveled + t >= maxDist` stops there), one above,
    x·(1 + 1e-9), and 2·x: a distance well beyond the hit, without which c5 — where most rays of
    the set miss everything and answer 1.0 at every distance — has 0.24 of its pairs at T == 0."""
    out = [np.inf, 0.0, -1.0, np.nan, 5e-324, bias / 2.0, bias, 2.0 * bias, DBL_MAX]
    for x in xs:
        out += [raysets.step(x, -1), x, raysets.step(x, 1), x * (1.0 + 1e-9), 2.0 * x]
    return out + list(extra)


def _table(sc, rays, bias=BIAS, extra=()):
    """dict: sc, base rays, and per pair rays [m, 6], dist [m], expected [m], ray index [m]."""
    orc = Oracle(sc)
    rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
    rr, dd, ii, ee, xs_all = [], [], [], [], []
    for i, r in enumerate(rays):
        xs = thresholds(orc, r, bias)
        xs_all.append(xs)
        for x in distances(xs, bias, extra):
            rr.append(r)
            dd.append(x)
            ii.append(i)
            ee.append(orc.transmittance(r, x, bias))
    t = dict(sc=sc, base=rays, bias=bias, thresholds=xs_all,
             rays=np.array(rr, np.float64).reshape(-1, 6), dist=np.array(dd, np.float64),
             expected=np.array(ee, np.float64), index=np.array(ii, np.int64))
    for k in ("base", "rays", "dist", "expected", "index"):
        t[k].setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def scene_table(name: str, bias: float = BIAS) -> dict:
    """The finite ray set of a raysets.SCENES scene with its distances and expected answers."""
    sc = raysets.scene(name)
    rays, _ = raysets.rayset(sc)
    if len(sc.triangle_array()) > MESH_TRIS:
        rays = rays[:MESH_RAYS]
    return _table(sc, rays, bias)


@functools.lru_cache(maxsize=None)
def grid_table(name: str) -> dict:
    """The raysets.CRAFTED grid sets (a BVH over coplanar, tying triangles)."""
    sc, rays, _ = raysets.CRAFTED[name]()
    return _table(sc, rays)


@functools.lru_cache(maxsize=None)
def nonfinite_table(name: str) -> dict:
    sc = raysets.scene(name)
    return _table(sc, raysets.nonfinite_rays(sc))


# ------------------------------------------------------------------ crafted sets
SHELL_COUNTS = (40, 70)   # 70: the sphere layout above 64
SHELL_HEIGHTS = (0.0, 0.5, 0.99, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 4.99, 5.5)


def shells_scene(n: int) -> SceneData:
    """n concentric spheres of transparency 1.0 around the origin, radii from 1 to 5, and an
    opaque sphere of radius 6 behind them at (20, 0, 0).  A ray along +x at height h crosses the
    shells of radius > h, two surfaces each: more than 32 of them use up the march's 64 steps
    before the opaque sphere is seen (T = 1); fewer let the march reach it (T = 0)."""
    sc = SceneData(raysets._cam(), name=f"shells{n}")
    for r in np.linspace(1.0, 5.0, n):
        sc.add_sphere((0.0, 0.0, 0.0), float(r), Material((0.9, 0.9, 1.0), transparency=1.0))
    sc.add_sphere((20.0, 0.0, 0.0), 6.0, Material((0.8, 0.3, 0.2)))
    sc.add_light((0.0, 30.0, 0.0), (1.0, 1.0, 1.0), 100.0)
    return sc


def shells_rays() -> np.ndarray:
    rows = []
    for k, h in enumerate(SHELL_HEIGHTS):
        z = (0.0, 0.125)[k % 2]
        rows.append([-10.0, h, z, 1.0, 0.0, 0.0])
        rows.append([-10.0, -h, z, 2.0, 0.0, 0.0])
    return np.array(rows, np.float64)


def crossed_shells(n: int, ray) -> int:
    """Shells whose radius exceeds the ray's distance from the x axis."""
    h = float(np.hypot(ray[1], ray[2]))
    return int((np.linspace(1.0, 5.0, n) > h).sum())


ROW_SPHERES = 12


def row_scene(transparencies) -> SceneData:
    """Twelve disjoint unit spheres along x (centres 0, 3, ..., 33) and an opaque plane behind
    them at x = 40.  transparencies: cycled over the spheres."""
    sc = SceneData(raysets._cam(), name="row")
    for k in range(ROW_SPHERES):
        tr = transparencies[k % len(transparencies)]
        sc.add_sphere((3.0 * k, 0.0, 0.0), 1.0, Material((0.9, 0.9, 1.0), transparency=tr))
    sc.add_plane((40.0, 0.0, 0.0), (-1.0, 0.0, 0.0), Material((0.8, 0.8, 0.8)))
    sc.add_light((0.0, 30.0, 0.0), (1.0, 1.0, 1.0), 100.0)
    return sc


def row_rays() -> np.ndarray:
    return np.array([[-5.0, 0.0, 0.0, 1.0, 0.0, 0.0],
                     [-5.0, 0.0, 0.0, 2.0, 0.0, 0.0],
                     [-5.0, 0.25, -0.125, 1.0, 0.0, 0.0],
                     [-5.0, 0.25, -0.125, 2.0, 0.0, 0.0],
                     [50.0, 0.0, 0.0, -1.0, 0.0, 0.0]], np.float64)   # from behind the plane


ROW_EXTRA = tuple(np.arange(0.5, 50.0, 0.75))


@functools.lru_cache(maxsize=None)
def crafted_table(name: str) -> dict:
    """shells40 / shells70, row (transparency 0.5: the T <= 1e-4 exit), row_clamp (0.9 and 1.5:
    the clamp to [0, 1]) and occlusion_sets.plane_at_zero (the t <= 0 step)."""
    if name.startswith("shells"):
        return _table(shells_scene(int(name[6:])), shells_rays(), extra=(20.0, 30.0))
    if name == "row":
        return _table(row_scene((0.5,)), row_rays(), extra=ROW_EXTRA)
    if name == "row_clamp":
        return _table(row_scene((0.9, 1.5)), row_rays(), extra=ROW_EXTRA)
    if name == "plane_at_zero":
        sc, rays = occlusion_sets.plane_at_zero()
        return _table(sc, rays, extra=(4.0, raysets.step(4.0, 1), 10.0))
    raise KeyError(name)


CRAFTED = ("shells40", "shells70", "row", "row_clamp", "plane_at_zero")


# ------------------------------------------------------------------ light tables
def light_scene(name: str) -> SceneData:
    return make_config(name, *raysets.SIZE) if name in ("c3", "c4") else raysets.scene(name)


def _dot(a, b):
    """Vec3::dot row by row: x·x' + y·y' + z·z', left to right."""
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def shadow_rays(points, lpos, bias: float):
    """directLightning's shadow ray from every point {p, normal} to the light at lpos, in the
    reference's order (Scene.h:81, 87-104): (rays [n, 6], max_dist [n], cast [n]) — cast is
    False where one of the three `continue`s skips the light (the answer is 0.0 there)."""
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 6)
    p, n_in = points[:, :3], points[:, 3:]
    with np.errstate(all="ignore"):
        ln = np.sqrt(_dot(n_in, n_in))
        normal = np.where((ln <= 1e-12)[:, None], 0.0, n_in / ln[:, None])   # Vec3::normalize
        v = np.asarray(lpos, np.float64)[None, :] - p
        dist = np.sqrt(_dot(v, v))
        L = v / dist[:, None]
        x = _dot(normal, L)
        ndl = np.where(0.0 < x, x, 0.0)                                       # std::max(0.0, x)
        cast = ~(dist <= 0.0) & ~(ndl <= 0.0) & ~(dist <= bias)
        rays = np.concatenate([p + normal * bias, L], axis=1)
        return rays, dist - bias, cast


def surface_points(sc: SceneData, rays) -> np.ndarray:
    """{hit point, normal facing the viewer} of the oracle's closest hits of `rays`: the rows
    that hit and are finite, the normal flipped against the ray as TraceRay flips it."""
    from oracle import pyoracle as po
    rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
    cl = po.closest_rays(sc, rays)
    keep = (cl[:, 0] != 0) & np.isfinite(cl).all(axis=1) & np.isfinite(rays).all(axis=1)
    cl, d = cl[keep], rays[keep, 3:]
    n = cl[:, 3:6]
    front = _dot(n, d) < 0.0
    return np.ascontiguousarray(np.concatenate([cl[:, 6:9], np.where(front[:, None], n, -n)], 1))


@functools.lru_cache(maxsize=None)
def light_table(name: str, bias: float = BIAS) -> dict:
    """dict: sc, points [n, 6], expected [n, n_lights]."""
    sc = light_scene(name)
    rays, _ = raysets.rayset(sc)
    return points_table(sc, surface_points(sc, rays), bias)


def points_table(sc: SceneData, pts, bias: float = BIAS) -> dict:
    """The expected [n, n_lights] of the points {p, normal}: the shadow rays formed in numpy, the
    three skips applied, one oracle_transmittance call for each of the rest."""
    orc = Oracle(sc)
    exp = np.zeros((len(pts), len(sc.lights)), np.float64)
    for l, (lpos, _, _) in enumerate(sc.lights):
        sr, md, cast = shadow_rays(pts, lpos, bias)
        for i in np.flatnonzero(cast):
            exp[i, l] = orc.transmittance(sr[i], md[i], bias)
    pts.setflags(write=False)
    exp.setflags(write=False)
    return dict(sc=sc, points=pts, expected=exp, bias=bias)


def same_bits(a, b) -> bool:
    """Equality of float64 bits (a NaN would show, and -0.0 is not 0.0)."""
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
