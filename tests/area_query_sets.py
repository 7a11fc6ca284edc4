"""Expected answers for the keyed queries (rt_scatter_rays_keyed, rt_direct_light_keyed,
rt_direct_light_rays_keyed, rt_light_transmittance_keyed: the per-level queries with the
build-defined area light served), shared by tests/test_area_queries_host.py (which checks them on
the CPU against the oracle's TraceRay and RenderImage) and tests/test_gpu_area_queries.py (which
runs them on the device).

The area light's part of directLightning is restated here in numpy, one IEEE operation per
operation of the oracle's loop (oracle/rt_oracle.c, `direct`) and in its order: every draw is one
pyoracle.u01 call under the key (seed, pixel, 0x10000 + (sample << 6) + depth, 2s | 2s + 1), the
sample point is (corner + edge_u*fu) + edge_v*fv, every shadow ray's T is one
oracle_transmittance call and every pow is math.pow.  Everything that does not involve the area
light is the existing restatements': direct_light_sets.expected for the point lights (whose two
accumulators the area samples continue), scatter_sets.level for the level's children,
transmittance_sets.points_table for the point lights' shadow rays.

Tables are cached per scene and key set: a reference is computed once and left unchanged.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import direct_light_sets as dl
import raysets
import scatter_sets as ss
import transmittance_sets as ts

BIAS = dl.BIAS
SEED = 0x5EED                       # rt_render_opts_default's, and the oracle's default
SCENES = ("c5", "glass_tri_area")
_dot = dl._dot
_normalize = dl._normalize

# The two key sets every table test runs under: the defaults (pixel = the element's index, sample
# 0, depth 0, the default seed) and explicit keys with every member away from its default.
EXPLICIT = dict(sample=3, depth=2, seed=0xC0FFEE1234)


def explicit_pixels(n: int) -> np.ndarray:
    return (np.arange(n, dtype=np.uint64) * np.uint64(1000003)) % np.uint64(1 << 40)


def key_set(mode: str, n: int) -> dict:
    """pixel [n] uint64, sample, depth, seed of the key set `mode` ("default" | "explicit")."""
    if mode == "default":
        return dict(pixel=np.arange(n, dtype=np.uint64), sample=0, depth=0, seed=SEED)
    return dict(pixel=explicit_pixels(n), **EXPLICIT)


def stream_of(sample: int, depth: int) -> int:
    return (0x10000 + (sample << 6) + depth) & 0xFFFFFFFF


def sample_points(sc, pixel, sample: int, depth: int, seed: int) -> np.ndarray:
    """The area light's sample points [n, samples, 3] of the elements keyed by pixel [n]."""
    from oracle import pyoracle as po
    al = sc.area_light
    k = int(round(math.sqrt(al.samples)))
    stream = stream_of(sample, depth)
    corner = np.asarray(al.corner, np.float64)
    eu, ev = np.asarray(al.edge_u, np.float64), np.asarray(al.edge_v, np.float64)
    out = np.empty((len(pixel), al.samples, 3), np.float64)
    for i, px in enumerate(pixel):
        for s in range(al.samples):
            r1 = np.float64(po.u01(seed, int(px), stream, 2 * s))
            r2 = np.float64(po.u01(seed, int(px), stream, 2 * s + 1))
            fu = (np.float64(s % k) + r1) / np.float64(k)
            fv = (np.float64(s // k) + r2) / np.float64(k)
            out[i, s] = (corner + eu * fu) + ev * fv
    return out


def _shadow(orc, p, normal, lpos, bias):
    """directLightning's shadow ray from every point to its own light point lpos [n, 3]
    (Scene.h:87-104): dist, L, ndl, cast (False where a `continue` skips) and T (0.0 there)."""
    with np.errstate(all="ignore"):
        v = lpos - p
        dist = np.sqrt(_dot(v, v))
        L = v / dist[:, None]
        x = _dot(normal, L)
        ndl = np.where(0.0 < x, x, 0.0)
        cast = ~(dist <= 0.0) & ~(ndl <= 0.0) & ~(dist <= bias)
        rays = np.concatenate([p + normal * bias, L], axis=1)
        md = dist - bias
    T = np.zeros(len(p), np.float64)
    for i in np.flatnonzero(cast):
        T[i] = orc.transmittance(rays[i], md[i], bias)
    return dist, L, ndl, cast, T


def light_columns(sc, points, pixel, sample=0, depth=0, seed=SEED, bias=BIAS) -> np.ndarray:
    """rt_light_transmittance_keyed: [n, n_lights + samples]."""
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 6)
    cols = [np.array(ts.points_table(ss.without_area_light(sc), points.copy(), bias)["expected"])]
    if sc.area_light is not None:
        orc = ts.Oracle(sc)
        normal = _normalize(points[:, 3:6])
        lp = sample_points(sc, pixel, sample, depth, seed)
        cols.append(np.stack([_shadow(orc, points[:, :3], normal, lp[:, s], bias)[4]
                              for s in range(sc.area_light.samples)], axis=1))
    return np.ascontiguousarray(np.concatenate(cols, axis=1))


def expected(sc, points, materials, pixel, sample=0, depth=0, seed=SEED, bias=BIAS) -> dict:
    """rt_direct_light_keyed: directLightning over the point lights (direct_light_sets.expected)
    continued over the area samples: radiance, diffuse, specular [n, 3], pow [n]."""
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 9)
    n = len(points)
    m = np.broadcast_to(np.asarray(materials, np.float64).reshape(-1, 7), (n, 7))
    base = dl.expected(ss.without_area_light(sc), points, m, bias)
    diff, spec, reached = np.array(base["diffuse"]), np.array(base["specular"]), np.array(base["pow"])
    al = sc.area_light
    if al is not None and n:
        orc = ts.Oracle(sc)
        p, view = points[:, :3], points[:, 6:]
        normal = _normalize(points[:, 3:6])
        lp = sample_points(sc, pixel, sample, depth, seed)
        li = np.float64(al.intensity) / np.float64(al.samples)
        emitted = np.asarray(al.color, np.float64) * li
        with np.errstate(all="ignore"):
            for s in range(al.samples):
                dist, L, ndl, cast, t = _shadow(orc, p, normal, lp[:, s], bias)
                use = cast & ~(t <= bias)
                scaled = emitted[None, :] * (1.0 / (dist * dist))[:, None]
                diff = np.where(use[:, None], diff + (scaled * ndl[:, None]) * t[:, None], diff)
                gate = use & (m[:, 5] <= 0.0) & (m[:, 4] > 0.0)
                H = _normalize(L + view)
                y = _dot(normal, H)
                ndh = np.where(0.0 < y, y, 0.0)
                reach = gate & (ndh > 0.0)
                sf = np.zeros(n, np.float64)
                for i in np.flatnonzero(reach):
                    sf[i] = _pow1(ndh[i], m[i, 3])
                spec = np.where(reach[:, None], spec + (scaled * sf[:, None]) * t[:, None], spec)
                reached |= reach
    with np.errstate(all="ignore"):
        radiance = m[:, :3] * diff + spec * m[:, 4:5]
    out = dict(radiance=radiance, diffuse=diff, specular=spec, pow=reached)
    for a in out.values():
        a.setflags(write=False)
    return out


def _pow1(x, y) -> float:
    try:
        return math.pow(x, y)
    except (OverflowError, ValueError):
        return float(np.float64(x) ** np.float64(y))


def expected_rays(sc, rays, pixel, sample=0, depth=0, seed=SEED, bias=BIAS) -> dict:
    """rt_direct_light_rays_keyed: `expected` at the oracle's closest hits, zeros on a miss;
    hit [n] marks the rays that hit."""
    rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
    n = len(rays)
    out = dict(radiance=np.zeros((n, 3)), diffuse=np.zeros((n, 3)), specular=np.zeros((n, 3)),
               pow=np.zeros(n, bool), hit=np.zeros(n, bool))
    h = dl.hits(sc, rays, finite_only=False) if n else None
    if h is not None and len(h["index"]):
        idx = h["index"]
        e = expected(sc, h["points"], h["materials"], np.asarray(pixel, np.uint64)[idx], sample,
                     depth, seed, bias)
        for k in ("radiance", "diffuse", "specular", "pow"):
            out[k][idx] = e[k]
        out["hit"][idx] = True
    for a in out.values():
        a.setflags(write=False)
    return out


def level(sc, rays, pixel, sample=0, depth=0, seed=SEED, bias=BIAS, terminal=False) -> dict:
    """rt_scatter_rays_keyed: scatter_sets.level (children, weights, flags, a miss's value) with
    the hits' value formed from the keyed localLight (Scene.h:169-173)."""
    rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
    out = {k: np.array(v) for k, v in ss.level(sc, rays, bias, terminal).items()}
    if sc.area_light is not None and not terminal and len(rays):
        h = dl.hits(sc, rays, finite_only=False)
        idx = h["index"]
        if len(idx):
            e = expected(sc, h["points"], h["materials"], np.asarray(pixel, np.uint64)[idx],
                         sample, depth, seed, bias)
            with np.errstate(all="ignore"):
                tr = ss._clamp(h["materials"][:, 5], 0.0, 1.0)
                out["value"][idx] = np.where(
                    (tr < 1.0)[:, None],
                    np.zeros((len(idx), 3)) + e["radiance"] * (1.0 - tr)[:, None], 0.0)
            out["pow_value"][idx] = e["pow"]
    for a in out.values():
        a.setflags(write=False)
    return out


def compose(sc, rays, depth: int, pixel=None, sample=0, seed=SEED, bias=BIAS, depth_key=None,
            _level: int = 0) -> np.ndarray:
    """Scene::TraceRay(ray, 0, bias) with maxRecursion = depth from `level` alone: level k is
    asked with depth = k (depth_key(k) when given) and its rays' ancestors' pixel keys."""
    rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
    pixel = np.arange(len(rays), dtype=np.uint64) if pixel is None else np.asarray(pixel, np.uint64)
    dk = _level if depth_key is None else depth_key(_level)
    if _level >= depth:
        return np.array(level(sc, rays, pixel, sample, dk, seed, bias, terminal=True)["value"])
    s = level(sc, rays, pixel, sample, dk, seed, bias)
    total = np.array(s["value"])
    with np.errstate(all="ignore"):
        for key, bit, w in (("refract_rays", ss.REFRACT, 0), ("reflect_rays", ss.REFLECT, 1)):
            live = (s["flags"] & bit) != 0
            if live.any():
                child = compose(sc, s[key][live], depth, pixel[live], sample, seed, bias,
                                depth_key, _level + 1)
                total[live] = total[live] + child * s["weights"][live, w:w + 1]
    return total


def frame_pixels(sc) -> np.ndarray:
    """pixel = y*W + x of raysets.camera_rays' rows."""
    return np.arange(sc.camera.width * sc.camera.height, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def table(name: str, mode: str) -> dict:
    """Every keyed entry's expected outputs on the scene's 648-ray set under the key set `mode`:
    sc, rays, keys, scatter (level), rays_dl (expected_rays), the closest hits' points and
    materials with points_dl / shared_dl (expected with the hits' own and with one shared
    material) and light_T (light_columns of the hits' {p, normal})."""
    sc = raysets.scene(name)
    rays, _ = raysets.rayset(sc)
    rays.setflags(write=False)
    keys = key_set(mode, len(rays))
    kw = dict(sample=keys["sample"], depth=keys["depth"], seed=keys["seed"])
    h = dl.hits(sc, rays, finite_only=False)
    hit_px = keys["pixel"][h["index"]]
    shared = np.array([[0.8, 0.7, 0.6, 16.0, 0.4, 0.0, 1.0]], np.float64)
    shared.setflags(write=False)
    t = dict(sc=sc, rays=rays, keys=keys, hits=h, hit_pixel=hit_px, shared=shared,
             scatter=level(sc, rays, keys["pixel"], **kw),
             rays_dl=expected_rays(sc, rays, keys["pixel"], **kw),
             points_dl=expected(sc, h["points"], h["materials"], hit_px, **kw),
             shared_dl=expected(sc, h["points"], shared, hit_px, **kw),
             light_T=light_columns(sc, h["points"][:, :6], hit_px, **kw))
    t["light_T"].setflags(write=False)
    return t


same_bits = ts.same_bits
within_bar = dl.within_bar


def matches(got, ref, pow_rows=None) -> bool:
    """got equals ref bit for bit, except on pow_rows (a row mask), held to within_bar."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        return False
    if pow_rows is None or not np.any(pow_rows):
        return same_bits(got, ref)
    rest = ~np.asarray(pow_rows, bool)
    return bool(same_bits(got[rest], ref[rest]) and within_bar(got[pow_rows], ref[pow_rows]).all())
