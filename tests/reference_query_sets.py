"""The questions put to the compiled reference for tests/golden/query_tables.npz: one list of
cases for tests/golden/make_golden.py --queries (which records what oracle/_ref/ref_harness
answers), tests/test_reference_queries.py (which holds the expected tables of the *_sets.py
modules and the oracle to those answers on the CPU) and tests/test_gpu_reference_queries.py (which
holds the device entries to them).

A case is one run of one harness mode: a key, the mode, a scene, the input arrays in the mode's
argument order, and the mode's trailing parameters.  Every input comes from the *_sets.py modules
the other tests use, so nothing drifts; the fixture stores the answers and a SHA-256 of the scene
text and of each input array, never the inputs.  Scenes without an area light only: the reference
has none.

    mode       inputs                       answer
    anybefore  rays [m,6], dist [m]         uint8 [m]       Scene::IntersectAnyBefore
    transmit   rays [m,6], dist [m]         float64 [m]     Scene::computeTransmittance
    direct     points [n,9], materials [n,7]  float64 [n,9] Scene::directLightning: radiance,
                                                            diffuse and specular accumulators
    trace      rays [n,6]                   float64 [n,3]   Scene::TraceRay(ray, 0, bias)
    closest    rays [n,6]                   float64 [n,9]   Scene::IntersectClosest
"""
from __future__ import annotations

import functools
import hashlib

import numpy as np

import direct_light_sets as dl
import occlusion_sets as oc
import raysets
import transmittance_sets as ts

BIAS = raysets.BIAS
FIXTURE = "query_tables.npz"
OCC_SCENES = ("c2", "sph300", "c1", "mirror", "glass", "mesh", "bigmesh")
OCC_NONFINITE = ("c2", "mesh")
TR_SCENES = OCC_SCENES
TR_NONFINITE = ("c2", "mesh")
TR_SHADOW_SCENES = ("c2", "c3", "c4", "glass", "mesh")
DL_SCENES = tuple(n for n in dl.LIGHT_SCENES if n != "glass_tri_area")
DL_PER_LIGHT = ("c3", "row")
TRACE_SCENES = ("c2", "c1", "mirror", "glass", "mesh")
TRACE_DEPTHS = (0, 1, 2, 3, 16)
COMPOSE_SCENES = ("glass", "mirror", "c1")
COMPOSE_DEPTHS = (1, 2, 3)
NONFINITE_RAY_SCENES = ("c2", "glass", "mesh")
PLANE_AT_ZERO_DIST = (10.0, np.inf, 4.0, raysets.step(4.0, 1))


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).hexdigest()


def scene_sha(sc) -> str:
    return hashlib.sha256(sc.to_text().encode()).hexdigest()


def _case(key, mode, sc, inputs, bias=BIAS, extra=()):
    inputs = tuple(np.ascontiguousarray(a, np.float64) for a in inputs)
    return dict(key=key, mode=mode, sc=sc, inputs=inputs, bias=bias, extra=tuple(extra))


# ------------------------------------------------------------------ the tables behind the cases
def occlusion_table(kind: str, name: str = "") -> dict:
    if kind == "scene":
        return oc.scene_table(name)
    if kind == "crafted":
        return oc.crafted_table(name)
    if kind == "nonfinite":
        return oc.nonfinite_table(name)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def plane_at_zero() -> dict:
    """occlusion_sets.plane_at_zero, every ray with each of PLANE_AT_ZERO_DIST, distance after
    distance: rows 4k..4k+3 are the four rays at distance k."""
    sc, base = oc.plane_at_zero()
    tp = oc.tpos(sc, base)
    rays = np.tile(base, (len(PLANE_AT_ZERO_DIST), 1))
    dist = np.repeat(np.array(PLANE_AT_ZERO_DIST, np.float64), len(base))
    return dict(sc=sc, base=base, tpos=tp, rays=rays, dist=dist, expected=np.tile(tp, 4) < dist)


def transmittance_table(kind: str, name: str) -> dict:
    if kind == "scene":
        return ts.scene_table(name)
    if kind == "grid":
        return ts.grid_table(name)
    if kind == "nonfinite":
        return ts.nonfinite_table(name)
    if kind == "crafted":
        return ts.crafted_table(name)
    raise KeyError(kind)


def shadow_case(name: str, l: int) -> dict:
    """The shadow rays directLightning casts from light_table(name)'s points to light l (the rows
    none of the three `continue`s skips): rows [k] of the points, rays, dist, and the table's
    transmittance for them."""
    t = ts.light_table(name)
    rays, md, cast = ts.shadow_rays(t["points"], t["sc"].lights[l][0], t["bias"])
    rows = np.flatnonzero(cast)
    return dict(sc=t["sc"], rows=rows, cast=cast, rays=rays[rows], dist=md[rows],
                expected=np.ascontiguousarray(t["expected"][rows, l]))


def direct_set(kind: str, name: str = "") -> dict:
    """dict with sc, points [n,9], materials [n,7] (broadcast) and the expected tables."""
    if kind == "own":
        s = dl.scene_set(name)
    elif kind == "spec":
        s = dl.scene_set(name, own_materials=False)
    elif kind == "row":
        s = dl.row_set()
    elif kind == "lowspec":
        s = dl.lowspec_set()
    elif kind == "bias_edge":
        s = dl.bias_edge_set()
    elif kind == "nonfinite":
        return nonfinite_direct(name)
    else:
        raise KeyError(kind)
    s = dict(s)
    s["materials"] = np.ascontiguousarray(np.broadcast_to(
        np.asarray(s["materials"], np.float64).reshape(-1, 7), (len(s["points"]), 7)))
    return s


@functools.lru_cache(maxsize=None)
def nonfinite_direct(name: str) -> dict:
    sc, pts, mats = dl.nonfinite_points(name)
    return dict(sc=sc, points=pts, materials=mats, bias=BIAS, **dl.expected(sc, pts, mats))


def direct_sets():
    """(key suffix, kind, name) of every direct-lighting set."""
    out = [(f"scene/{n}/own", "own", n) for n in DL_SCENES]
    out += [(f"scene/{n}/spec", "spec", n) for n in dl.SPEC_SCENES]
    out += [("row", "row", ""), ("lowspec", "lowspec", ""), ("bias_edge", "bias_edge", ""),
            ("nonfinite/c2", "nonfinite", "c2")]
    return out


def per_light_set(name: str) -> dict:
    return direct_set("row") if name == "row" else direct_set("own", name)


# ------------------------------------------------------------------ the cases
def cases():
    """Every case, in the fixture's order."""
    for n in OCC_SCENES:
        t = occlusion_table("scene", n)
        yield _case(f"occ/scene/{n}", "anybefore", t["sc"], (t["rays"], t["dist"]))
    for n in raysets.CRAFTED:
        t = occlusion_table("crafted", n)
        yield _case(f"occ/crafted/{n}", "anybefore", t["sc"], (t["rays"], t["dist"]))
    for n in OCC_NONFINITE:
        t = occlusion_table("nonfinite", n)
        yield _case(f"occ/nonfinite/{n}", "anybefore", t["sc"], (t["rays"], t["dist"]))
    t = plane_at_zero()
    yield _case("occ/plane_at_zero", "anybefore", t["sc"], (t["rays"], t["dist"]))

    for kind, names in (("scene", TR_SCENES), ("grid", ts.BVH_GRIDS), ("nonfinite", TR_NONFINITE),
                        ("crafted", ts.CRAFTED)):
        for n in names:
            t = transmittance_table(kind, n)
            yield _case(f"tr/{kind}/{n}", "transmit", t["sc"], (t["rays"], t["dist"]), t["bias"])
    for n in TR_SHADOW_SCENES:
        for l in range(len(ts.light_scene(n).lights)):
            s = shadow_case(n, l)
            yield _case(f"tr/shadow/{n}/{l}", "transmit", s["sc"], (s["rays"], s["dist"]))

    for suffix, kind, n in direct_sets():
        s = direct_set(kind, n)
        yield _case(f"dl/{suffix}", "direct", s["sc"], (s["points"], s["materials"]), s["bias"])
    for n in DL_PER_LIGHT:
        s = per_light_set(n)
        for l in range(len(s["sc"].lights)):
            yield _case(f"dl/light/{n}/{l}", "direct", s["sc"], (s["points"], s["materials"]),
                        s["bias"], extra=(l,))

    for n in TRACE_SCENES:
        sc = raysets.scene(n)
        rays, _ = raysets.rayset(sc)
        for d in TRACE_DEPTHS:
            yield _case(f"trace/{n}/{d}", "trace", sc, (rays,), extra=(d,))
    for n in raysets.CRAFTED:
        sc, rays, _ = raysets.CRAFTED[n]()
        yield _case(f"closest/crafted/{n}", "closest", sc, (rays,))
    for n in NONFINITE_RAY_SCENES:
        sc = raysets.scene(n)
        rays = raysets.nonfinite_rays(sc)
        yield _case(f"closest/nonfinite/{n}", "closest", sc, (rays,))
        yield _case(f"trace/nonfinite/{n}", "trace", sc, (rays,))


def case_hashes(c: dict) -> np.ndarray:
    """What the fixture keeps of a case's inputs: the SHA-256 of the scene text, of each input
    array, and the trailing parameters as text."""
    return np.array([scene_sha(c["sc"]), *map(sha, c["inputs"]),
                     " ".join(map(repr, (c["bias"], *c["extra"])))])


def check_inputs(golden: dict, c: dict):
    """The generator of a case still makes what the reference was asked."""
    want = case_hashes(c)
    have = golden[c["key"] + "#in"]
    names = ["scene"] + [f"input {k}" for k in range(len(c["inputs"]))] + ["parameters"]
    for n, w, h in zip(names, want, have):
        assert str(w) == str(h), f"{c['key']}: {n} drifted from the golden"
    assert len(want) == len(have), c["key"]


def canonical_bits(a) -> np.ndarray:
    return dl.canonical_bits(a)


def same(a, b) -> bool:
    """Bit for bit, a NaN equal to a NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(canonical_bits(a), canonical_bits(b))
