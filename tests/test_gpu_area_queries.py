"""The keyed queries on the device (the keyed_ kernels of rt_scatter.hip, rt_direct.hip and
rt_transmit.hip, each the un-keyed kernel's body with the area light on): rt_scatter_rays_keyed,
rt_direct_light_keyed, rt_direct_light_rays_keyed, rt_light_transmittance_keyed and their _device
twins — the per-level queries with the build-defined area light served under keys the caller
supplies — on the two small area-light scenes of tests/raysets.py (c5: 16 samples, no point
light, no pow; glass_tri_area: 4 samples, one point light, glass, mirrors and pow).  The un-keyed
entries, which share that body, are held to ignore the light.

The comparator is tests/area_query_sets.py, which tests/test_area_queries_host.py holds to the
oracle's TraceRay and RenderImage on the CPU; the second group below compares with the oracle
directly.  Values are compared as bits where directLightning does not reach std::pow and within
1e-12 * max(1, |ref|) where it does; child rays, flags, a miss's value and every transmittance
as bits."""
import os
import subprocess

import numpy as np
import pytest
import torch

import area_query_sets as aq
import direct_light_sets as dl
import raysets
import scatter_sets as ss
from raytracingengine_amd import capi
from raytracingengine_amd.configs import make_config
from test_gpu_accumulate import CYCLIC
from test_gpu_scatter import assert_outputs_same, assert_same, assert_table, bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "bin", "area_light_scenefile")
SIZES = (0, 1, 63, 64, 65, 255, 256, 257)
MODES = ("default", "explicit")
GUARD = 64
FILL = -7.25
FILL_U8 = 0xA5
DL_KEYS = ("radiance", "diffuse", "specular")


def call_keys(keys, rows=None):
    """The keyword arguments of a key set of area_query_sets.  The default set over a whole ray
    set goes in as no keys at all (pixel = None: the element's index, the default seed); every
    other call spells its members out — `rows`: the elements are those rows of the ray set (the
    points of its hits), which keep their rays' keys."""
    if rows is None and (keys["seed"], keys["sample"], keys["depth"]) == (aq.SEED, 0, 0) \
            and np.array_equal(keys["pixel"], np.arange(len(keys["pixel"]), dtype=np.uint64)):
        return dict(area_keys=capi.AreaKeys())
    px = keys["pixel"] if rows is None else keys["pixel"][rows]
    return dict(area_keys=capi.AreaKeys(px, keys["sample"], keys["depth"]), seed=keys["seed"])


def assert_dl(got, ref, what):
    """A direct-light answer against area_query_sets.expected[_rays]: the diffuse accumulator as
    bits everywhere, the other two as bits where pow is not reached, within the bar where it is."""
    exact = ~ref["pow"]
    assert_same(got["diffuse"], ref["diffuse"], (what, "diffuse"))
    for k in ("radiance", "specular"):
        assert got[k].shape == ref[k].shape and got[k].dtype == np.float64, (what, k)
        assert_same(got[k][exact], ref[k][exact], (what, k, "no pow"))
        ok = dl.within_bar(got[k], ref[k])
        assert ok.all(), (what, k, np.argwhere(~ok)[:4])


def shading_points(cl, rays):
    """TraceRay's {hit point, flipped normal, view} and materials of the rows of a CH_ALL answer
    that hit (Scene.h:144-147), as direct_light_sets.hits forms them from the oracle's."""
    idx = np.flatnonzero(cl["prim"][:, 0] != 0)
    inc = dl._normalize(rays[idx, 3:])
    n = cl["normal"][idx]
    with np.errstate(all="ignore"):
        front = dl._dot(n, inc) < 0.0
    pts = np.concatenate([cl["point"][idx], np.where(front[:, None], n, -n), -inc], axis=1)
    return idx, np.ascontiguousarray(pts), np.ascontiguousarray(cl["material"][idx])


@pytest.fixture(scope="module")
def world(ctx, oracle):
    """Per scene, made once and left unchanged: the scene on the device, its rays and closest
    hits, and per key set every keyed entry's host answer."""
    cache = {}

    def get(name):
        if name not in cache:
            sc = raysets.scene(name)
            rays, _ = raysets.rayset(sc)
            rays.setflags(write=False)
            ds = ctx.scene(sc)
            idx, pts, mats = shading_points(ds.closest(rays), rays)
            w = dict(sc=sc, rays=rays, ds=ds, index=idx, points=pts, materials=mats, got={})
            for mode in MODES:
                keys = aq.key_set(mode, len(rays))
                kw, hkw = call_keys(keys), call_keys(keys, idx)
                w["got"][mode] = dict(
                    scatter=ds.scatter(rays, capi.SC_ALL, **kw),
                    rays_dl=ds.direct_light_rays(rays, capi.DL_ALL, **kw),
                    points_dl=ds.direct_light(pts, mats, capi.DL_ALL, **hkw),
                    light_T=ds.light_transmittance(pts[:, :6], **hkw))
            cache[name] = w
        return cache[name]
    yield get
    for w in cache.values():
        w["ds"].close()


# ------------------------------------------------------------------ 1. tables
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", aq.SCENES)
def test_tables(world, name, mode):
    w, t = world(name), aq.table(name, mode)
    got, ds = w["got"][mode], w["ds"]
    n, al = len(t["rays"]), t["sc"].area_light
    assert_table(got["scatter"], t["scatter"], (name, mode))
    hit = (got["scatter"]["flags"] & 1) != 0
    plain = ds.scatter(t["rays"], capi.SC_VALUE)["value"]
    matters = int((bits(plain) != bits(got["scatter"]["value"])).any(axis=1).sum())
    print(f"{name}/{mode}: {hit.sum()} hits, the area light changes {matters} values")
    assert hit.sum() >= 100 and (~hit).sum() >= 30 and matters >= 50
    assert_dl(got["rays_dl"], t["rays_dl"], (name, mode, "rays"))
    assert np.array_equal(hit, t["rays_dl"]["hit"])
    # the device's closest hits are the oracle's, so the point tables apply row for row
    assert_same(w["points"], t["hits"]["points"], (name, "points"))
    assert_same(w["materials"], t["hits"]["materials"], (name, "materials"))
    assert_dl(got["points_dl"], t["points_dl"], (name, mode, "points"))
    shared = ds.direct_light(w["points"], t["shared"], capi.DL_ALL, **call_keys(t["keys"], w["index"]))
    assert_dl(shared, t["shared_dl"], (name, mode, "shared material"))
    assert got["light_T"].shape == (len(w["index"]), len(t["sc"].lights) + al.samples)
    assert_same(got["light_T"], t["light_T"], (name, mode, "light_T"))
    soft = got["light_T"][:, -al.samples:].mean(axis=1)
    assert ((soft > 0.0) & (soft < 1.0)).sum() >= 10, "no penumbra in the set"
    if not raysets.SCENES[name]["pow"]:
        assert not t["scatter"]["pow_value"].any() and not t["rays_dl"]["pow"].any()
    assert n == 648


def test_key_sets_differ(world):
    """The explicit keys draw other sample points than the defaults."""
    for name in aq.SCENES:
        a, b = (world(name)["got"][m] for m in MODES)
        assert not dl.same_bits(a["scatter"]["value"], b["scatter"]["value"])
        assert not dl.same_bits(a["light_T"], b["light_T"])
        assert_same(a["scatter"]["flags"], b["scatter"]["flags"], name)


# ------------------------------------------------------------------ 2. against the oracle
def test_level_is_the_oracle_on_c5(world, oracle):
    w = world("c5")
    ref, _, _ = oracle.trace_rays(w["sc"], w["rays"], max_recursion=1)
    off, _, _ = oracle.trace_rays(w["sc"], w["rays"], max_recursion=1, use_area_light=False)
    assert int((ref != off).any(axis=1).sum()) >= 50
    assert_same(w["got"]["default"]["scatter"]["value"], ref, "c5 level")


def test_composition_is_trace_rays(world, oracle):
    w = world("glass_tri_area")
    ds, rays = w["ds"], w["rays"]
    ref, _, _ = oracle.trace_rays(w["sc"], rays, max_recursion=3)
    off, _, _ = oracle.trace_rays(w["sc"], rays, max_recursion=3, use_area_light=False)
    assert int((ref != off).any(axis=1).sum()) >= 300
    got = capi.compose_trace(ds, rays, 3, area_keys=capi.AreaKeys())
    assert dl.within_bar(got, ref).all()
    assert dl.within_bar(got, ds.trace_rays(rays, max_recursion=3)).all()
    # without keys the composition is the scene without its area light
    assert not dl.within_bar(capi.compose_trace(ds, rays, 3), ref).all()


def test_composition_is_the_frame(world, oracle):
    w = world("glass_tri_area")
    ds, sc = w["ds"], w["sc"]
    ref, _, _ = oracle.render(sc, max_recursion=3)
    off, _, _ = oracle.render(sc, max_recursion=3, use_area_light=False)
    assert int((ref != off).any(axis=2).sum()) >= 192
    cam = ds.camera_rays(0)
    assert_same(cam, raysets.camera_rays(sc), "camera rays")
    got = capi.compose_trace(ds, cam, 3, area_keys=capi.AreaKeys(aq.frame_pixels(sc)))
    assert dl.within_bar(got.reshape(ref.shape), ref).all()
    frame = ds.render(hdr64=True, max_recursion=3)["hdr64"]
    assert dl.within_bar(got.reshape(frame.shape), frame).all()


def _cyclic_rows(height):
    b, stride = CYCLIC["row_block"], CYCLIC["row_block"] * CYCLIC["row_cycle"]
    return [y for s in range(CYCLIC["row_begin"], height, stride) for y in range(s, min(s + b, height))]


@pytest.mark.parametrize("rows", ("full", "cyclic"))
def test_frame_from_its_samples(ctx, oracle, rows):
    """c5 at 24x16 with four AA samples, folded on the device from four keyed scatter calls on
    camera_rays_device(s) under the keys (y_image*W + x, s, 0): render's frame, bit for bit."""
    sc = make_config("c5", 24, 16, aa=4)
    w, h = sc.camera.width, sc.camera.height
    kw = {} if rows == "full" else CYCLIC
    ys = list(range(h)) if rows == "full" else _cyclic_rows(h)
    assert rows == "full" or ys == [2, 3, 8, 9, 14, 15]
    pix = torch.tensor([y * w + x for y in ys for x in range(w)], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ds = ctx.scene(sc)
    try:
        total = None
        for s in range(4):
            v = ds.scatter_device(ds.camera_rays_device(s, **kw), capi.SC_VALUE,
                                  area_keys=capi.AreaKeys(pix, s, 0))["value"]
            ctx.synchronize()
            total = (torch.zeros_like(v) + v) if total is None else total + v
        got = (total / 4.0).cpu().numpy()
        frame = ds.render(hdr64=True, **kw)["hdr64"]
        assert_same(got, frame.reshape(-1, 3), ("c5 aa=4", rows, "render"))
        ref, _, _ = oracle.render(sc)
        off, _, _ = oracle.render(sc, use_area_light=False)
        assert int((ref[ys] != off[ys]).any(axis=2).sum()) >= 10
        assert_same(got, ref[ys].reshape(-1, 3), ("c5 aa=4", rows, "oracle"))
    finally:
        ds.close()


# ------------------------------------------------------------------ 3. the key travels with its element
def _all_entries(ds, rays, pts, mats, ray_kw, pt_kw):
    """Every keyed entry's host answer as one flat dict."""
    out = {f"sc.{k}": v for k, v in ds.scatter(rays, capi.SC_ALL, **ray_kw).items()}
    out.update({f"rays.{k}": v for k, v in ds.direct_light_rays(rays, capi.DL_ALL, **ray_kw).items()})
    out.update({f"pts.{k}": v for k, v in ds.direct_light(pts, mats, capi.DL_ALL, **pt_kw).items()})
    out["light_T"] = ds.light_transmittance(pts[:, :6], **pt_kw)
    return out


@pytest.mark.parametrize("name", aq.SCENES)
def test_permutation(world, name):
    w = world(name)
    keys = aq.key_set("explicit", len(w["rays"]))
    got = w["got"]["explicit"]
    rng = np.random.default_rng(7)
    pr, pp = rng.permutation(len(w["rays"])), rng.permutation(len(w["index"]))
    ray_keys = dict(keys, pixel=keys["pixel"][pr])
    pt_keys = dict(keys, pixel=keys["pixel"][w["index"]][pp])
    res = _all_entries(w["ds"], w["rays"][pr], w["points"][pp], w["materials"][pp],
                       call_keys(ray_keys), call_keys(pt_keys))
    for k, v in got["scatter"].items():
        assert_same(res[f"sc.{k}"], v[pr], (name, k))
    for k in DL_KEYS:
        assert_same(res[f"rays.{k}"], got["rays_dl"][k][pr], (name, "rays", k))
        assert_same(res[f"pts.{k}"], got["points_dl"][k][pp], (name, "points", k))
    assert_same(res["light_T"], got["light_T"][pp], (name, "light_T"))


@pytest.mark.parametrize("n", SIZES)
def test_prefixes_without_keys(world, n):
    """pixel = None: element i draws with pixel = i, so rays[:n] gives the full call's first n
    rows, around the wave and workgroup sizes."""
    w = world("glass_tri_area")
    got = w["got"]["default"]
    kw = dict(area_keys=capi.AreaKeys())
    res = _all_entries(w["ds"], w["rays"][:n], w["points"][:n], w["materials"][:n], kw, kw)
    for k, v in got["scatter"].items():
        assert_same(res[f"sc.{k}"], v[:n], (n, k))
    for k in DL_KEYS:
        assert_same(res[f"rays.{k}"], got["rays_dl"][k][:n], (n, "rays", k))
    # the points of the default table are keyed by their ray's index: ask the prefix that way
    pk = dict(area_keys=capi.AreaKeys(w["index"][:n].astype(np.uint64)))
    pts = w["ds"].direct_light(w["points"][:n], w["materials"][:n], capi.DL_ALL, **pk)
    for k in DL_KEYS:
        assert_same(pts[k], got["points_dl"][k][:n], (n, "points", k))
    assert_same(w["ds"].light_transmittance(w["points"][:n, :6], **pk), got["light_T"][:n], n)
    assert res["light_T"].shape == (n, got["light_T"].shape[1])


@pytest.mark.parametrize("name", aq.SCENES)
def test_repeats(world, name):
    """The copies of ray 0 draw under other pixel keys (their indices) and differ from it
    somewhere; given ray 0's key they give ray 0's bytes."""
    w = world(name)
    rays, got = w["rays"], w["got"]["default"]["scatter"]
    rep = raysets.repeat_indices(len(rays))
    assert (got["flags"][0] & 1) != 0, "ray 0 misses: nothing to draw"
    assert any(got["value"][i].tobytes() != got["value"][0].tobytes() for i in rep), name
    same = w["ds"].scatter(rays[rep], capi.SC_ALL, area_keys=capi.AreaKeys(np.zeros(len(rep), np.uint64)))
    for k, v in same.items():
        for j in range(len(rep)):
            assert v[j].tobytes() == got[k][0].tobytes(), (name, k, j)


# ------------------------------------------------------------------ 4. consistency inside the family
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", aq.SCENES)
def test_consistent_inside_the_family(world, name, mode):
    w = world(name)
    got = w["got"][mode]
    sc, rd, pd = got["scatter"], got["rays_dl"], got["points_dl"]
    hit = (sc["flags"] & 1) != 0
    idx = w["index"]
    assert np.array_equal(np.flatnonzero(hit), idx)
    with np.errstate(all="ignore"):
        tr = ss._clamp(w["materials"][:, 5], 0.0, 1.0)
        value = np.where((tr < 1.0)[:, None],
                         np.zeros((len(idx), 3)) + rd["radiance"][idx] * (1.0 - tr)[:, None], 0.0)
    assert_same(sc["value"][idx], value, (name, mode, "value from direct_light_rays"))
    for k in DL_KEYS:
        assert_same(pd[k], rd[k][idx], (name, mode, "points == rays", k))
        assert not bits(rd[k][~hit]).any()
    plain = w["ds"].scatter(w["rays"], capi.SC_ALL & ~capi.SC_VALUE)
    for k, v in plain.items():
        assert_same(sc[k], v, (name, mode, "children do not depend on the keys", k))
    # a terminal level is the sky, whatever the keys
    term = w["ds"].scatter(w["rays"], capi.SC_ALL, terminal=True, **call_keys(aq.key_set(mode, 648)))
    assert_outputs_same(term, w["ds"].scatter(w["rays"], capi.SC_ALL, terminal=True), (name, mode))


# ------------------------------------------------------------------ 5. no area light
@pytest.mark.parametrize("name", ("c2", "glass", "glass_tri_area"))
def test_no_area_light_is_the_sibling(ctx, oracle, name):
    sc = ss.without_area_light(raysets.scene(name))
    assert sc.area_light is None
    rays, _ = raysets.rayset(sc)
    keys = aq.key_set("explicit", len(rays))
    ds = ctx.scene(sc)
    try:
        idx, pts, mats = shading_points(ds.closest(rays), rays)
        assert len(idx) >= 100
        for kw, hkw in ((call_keys(keys), call_keys(keys, idx)),
                        (dict(area_keys=capi.AreaKeys()),) * 2):
            assert_outputs_same(ds.scatter(rays, capi.SC_ALL, **kw), ds.scatter(rays, capi.SC_ALL), name)
            assert_outputs_same(ds.direct_light_rays(rays, capi.DL_ALL, **kw),
                                ds.direct_light_rays(rays, capi.DL_ALL), name)
            assert_outputs_same(ds.direct_light(pts, mats, capi.DL_ALL, **hkw),
                                ds.direct_light(pts, mats, capi.DL_ALL), name)
            a, b = ds.light_transmittance(pts[:, :6], **hkw), ds.light_transmittance(pts[:, :6])
            assert a.shape == (len(idx), len(sc.lights))
            assert_same(a, b, name)
    finally:
        ds.close()


def _unkeyed_host(ds, w, shared):
    """Every un-keyed host entry's answer on the rays and hit points of w, as one flat dict."""
    rays, pts = w["rays"], w["points"]
    out = {"light_T": ds.light_transmittance(pts[:, :6]),
           "sc.value": ds.scatter(rays, capi.SC_VALUE)["value"]}
    for who, res in (("rays", ds.direct_light_rays(rays, capi.DL_ALL)),
                     ("pts", ds.direct_light(pts, w["materials"], capi.DL_ALL)),
                     ("shared", ds.direct_light(pts, shared, capi.DL_ALL))):
        out.update({f"{who}.{k}": v for k, v in res.items()})
    return out


def _unkeyed_device(ctx, ds, w, shared):
    """The same dict from the _device entries."""
    d_rays = torch.from_numpy(w["rays"].copy()).cuda()
    d_pts = torch.from_numpy(w["points"].copy()).cuda()
    d_mats = torch.from_numpy(w["materials"].copy()).cuda()
    torch.cuda.synchronize()
    out = {"light_T": ds.light_transmittance_device(d_pts[:, :6].contiguous()),
           "sc.value": ds.scatter_device(d_rays, capi.SC_VALUE)["value"]}
    for who, res in (("rays", ds.direct_light_rays_device(d_rays, capi.DL_ALL)),
                     ("pts", ds.direct_light_device(d_pts, d_mats, capi.DL_ALL)),
                     ("shared", ds.direct_light_device(d_pts, shared, capi.DL_ALL))):
        out.update({f"{who}.{k}": v for k, v in res.items()})
    ctx.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", aq.SCENES)
def test_unkeyed_entries_ignore_the_area_light(ctx, world, name):
    """The un-keyed kernels are the keyed kernels' text with the area light switched off: on a
    scene with its area light attached every un-keyed entry, host and _device, answers with the
    bits it gives on the same scene built without the light.  The keyed radiance differs from the
    un-keyed one on at least 50 rays, so the light would show."""
    w = world(name)
    sc, ds = w["sc"], w["ds"]
    shared = aq.table(name, "default")["shared"]
    bare_sc = ss.without_area_light(sc)
    assert sc.area_light is not None and bare_sc.area_light is None
    bare = ctx.scene(bare_sc)
    try:
        want = _unkeyed_host(bare, w, shared)
        assert want["light_T"].shape == (len(w["index"]), len(sc.lights))
        assert_outputs_same(_unkeyed_host(ds, w, shared), want, (name, "host"))
        assert_outputs_same(_unkeyed_device(ctx, ds, w, shared), want, (name, "device, area light"))
        assert_outputs_same(_unkeyed_device(ctx, bare, w, shared), want, (name, "device, none"))
    finally:
        bare.close()
    keyed = w["got"]["default"]["rays_dl"]["radiance"]
    differ = int((bits(keyed) != bits(want["rays.radiance"])).any(axis=1).sum())
    print(f"{name}: the area light changes the radiance of {differ} of {len(keyed)} rays")
    assert len(keyed) == 648 and differ >= 50


# ------------------------------------------------------------------ 6. device forms
def _guarded(shape, dtype=torch.float64):
    n = int(np.prod(shape))
    fill = FILL_U8 if dtype == torch.uint8 else FILL
    full = torch.full((2 * GUARD + n,), fill, dtype=dtype, device="cuda")
    return full, full[GUARD:GUARD + n]


def _check_guarded(full, shape, want, what):
    raw = full.cpu().numpy()
    n = int(np.prod(shape))
    fill = FILL_U8 if raw.dtype == np.uint8 else FILL
    assert (raw[:GUARD] == fill).all() and (raw[GUARD + n:] == fill).all(), (what, "guard")
    assert_same(raw[GUARD:GUARD + n].reshape(shape), want, what)


def _device_forms(ctx, w, n, mode):
    """Every _device entry on rows [:n] into caller-provided tensors with guard zones, against
    the host entries' rows."""
    ds = w["ds"]
    keys = aq.key_set(mode, len(w["rays"]))
    got = w["got"][mode]
    d_rays = torch.from_numpy(w["rays"][:n].copy()).cuda()
    d_pts = torch.from_numpy(w["points"][:n].copy()).cuda()
    d_pn = d_pts[:, :6].contiguous()
    d_mats = torch.from_numpy(w["materials"][:n].copy()).cuda()
    explicit = mode == "explicit"

    def dev_keys(px):
        if not explicit and px is None:
            return dict(area_keys=capi.AreaKeys())
        t = torch.from_numpy(np.asarray(px, np.uint64).view(np.int64).copy()).cuda()
        return dict(area_keys=capi.AreaKeys(t, keys["sample"], keys["depth"]), seed=keys["seed"])
    ray_kw = dev_keys(keys["pixel"][:n] if explicit else None)
    pt_kw = dev_keys(keys["pixel"][w["index"][:n]])
    widths = {"value": 3, "refract_rays": 6, "reflect_rays": 6, "weights": 2}
    sc_full, sc_view = {}, {}
    for k, width in widths.items():
        sc_full[k], sc_view[k] = _guarded((n, width))
    sc_full["flags"], sc_view["flags"] = _guarded((n,), torch.uint8)
    dl_bufs = {who: {k: _guarded((n, 3)) for k in DL_KEYS} for who in ("rays", "pts")}
    cols = got["light_T"].shape[1]
    lt_full, lt_view = _guarded((n, cols))
    torch.cuda.synchronize()
    res = ds.scatter_device(d_rays, capi.SC_ALL, out=sc_view, **ray_kw)
    assert all(res[k] is sc_view[k] for k in sc_view)
    ds.direct_light_rays_device(d_rays, capi.DL_ALL, out={k: v[1] for k, v in dl_bufs["rays"].items()},
                                **ray_kw)
    ds.direct_light_device(d_pts, d_mats, capi.DL_ALL, out={k: v[1] for k, v in dl_bufs["pts"].items()},
                           **pt_kw)
    ds.light_transmittance_device(d_pn, out=lt_view, **pt_kw)
    ctx.synchronize()
    for k, width in widths.items():
        _check_guarded(sc_full[k], (n, width), got["scatter"][k][:n], (mode, n, k))
    _check_guarded(sc_full["flags"], (n,), got["scatter"]["flags"][:n], (mode, n, "flags"))
    for k in DL_KEYS:
        _check_guarded(dl_bufs["rays"][k][0], (n, 3), got["rays_dl"][k][:n], (mode, n, "rays", k))
        _check_guarded(dl_bufs["pts"][k][0], (n, 3), got["points_dl"][k][:n], (mode, n, "pts", k))
    _check_guarded(lt_full, (n, cols), got["light_T"][:n], (mode, n, "light_T"))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", (0, 65, 300))
def test_device_forms(ctx, world, n, mode):
    _device_forms(ctx, world("glass_tri_area"), n, mode)


def test_device_forms_c5_and_new_tensors(ctx, world):
    w = world("c5")
    _device_forms(ctx, w, len(w["index"]), "explicit")
    d_rays = torch.from_numpy(w["rays"].copy()).cuda()
    torch.cuda.synchronize()
    res = w["ds"].scatter_device(d_rays, capi.SC_ALL, area_keys=capi.AreaKeys())
    ctx.synchronize()
    assert_outputs_same({k: v.cpu().numpy() for k, v in res.items()}, w["got"]["default"]["scatter"], "c5")
    with pytest.raises(ValueError):   # host keys given to a device entry, the wrong type, the wrong count
        w["ds"].scatter_device(d_rays, area_keys=capi.AreaKeys(np.arange(648, dtype=np.uint64)))
    with pytest.raises(ValueError):
        w["ds"].scatter_device(d_rays, area_keys=capi.AreaKeys(torch.zeros(648, device="cuda")))
    with pytest.raises(ValueError):
        w["ds"].scatter_device(d_rays, area_keys=capi.AreaKeys(
            torch.zeros(647, dtype=torch.int64, device="cuda")))


def test_device_entries_on_a_caller_stream(world, oracle):
    """On a stream set through rt_context_set_stream the answers are there once that stream has
    synchronised."""
    w0 = world("glass_tri_area")
    keys = aq.key_set("explicit", len(w0["rays"]))
    with capi.Context(0) as c:
        ds = c.scene(w0["sc"])
        stream = torch.cuda.Stream()
        c.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            d_rays = torch.from_numpy(w0["rays"].copy()).to("cuda")
            px = torch.from_numpy(keys["pixel"].view(np.int64).copy()).to("cuda")
            kw = dict(area_keys=capi.AreaKeys(px, keys["sample"], keys["depth"]), seed=keys["seed"])
            a = ds.scatter_device(d_rays, capi.SC_ALL, **kw)
            b = ds.direct_light_rays_device(d_rays, capi.DL_ALL, **kw)
        stream.synchronize()
        got = w0["got"]["explicit"]
        assert_outputs_same({k: v.cpu().numpy() for k, v in a.items()}, got["scatter"], "stream")
        assert_outputs_same({k: v.cpu().numpy() for k, v in b.items()}, got["rays_dl"], "stream")
        c.set_stream(None)
        ds.close()


# ------------------------------------------------------------------ 7. errors on a live context
def test_errors_write_nothing(ctx, world):
    w = world("glass_tri_area")
    ds, n = w["ds"], 64
    rays, pts, mats = w["rays"][:n], w["points"][:n], w["materials"][:n]
    px = np.arange(n, dtype=np.uint64)

    def fresh(kind):
        res, ptrs = capi._outputs(kind, capi.SC_ALL if kind == "SC" else capi.DL_ALL, n)
        for v in res.values():
            v.fill(FILL_U8 if v.dtype == np.uint8 else FILL)
        return res, ptrs

    def untouched(res):
        return all((v == (FILL_U8 if v.dtype == np.uint8 else FILL)).all() for v in res.values())
    cases = (("depth", dict(area_keys=capi.AreaKeys(px, 0, 64))),
             ("sample", dict(area_keys=capi.AreaKeys(px, 0x01000000, 0))))
    for text, kw in cases:
        for call in (lambda: ds.scatter(rays, **kw), lambda: ds.direct_light_rays(rays, **kw),
                     lambda: ds.direct_light(pts, mats, **kw),
                     lambda: ds.light_transmittance(pts[:, :6], **kw)):
            with pytest.raises(capi.RtError) as e:
                call()
            assert e.value.status == capi.RT_ERR_INVALID_ARG and text in str(e.value)
    # through the entries themselves: outputs that must stay as they were
    import ctypes
    lib = capi.load_library()
    o = capi.default_opts()
    h, s = ctx.handle, ds._h
    good = capi.AreaKeysRec(px.ctypes.data, 0, 0)
    for rec, rays_ptr, outputs in ((capi.AreaKeysRec(px.ctypes.data, 0, 64), rays.ctypes.data, None),
                                   (capi.AreaKeysRec(px.ctypes.data, 0x01000000, 0), rays.ctypes.data, None),
                                   (good, None, None),            # keys, but NULL rays with n > 0
                                   (good, rays.ctypes.data, 0x40 | 1)):   # an unknown output bit
        res, ptrs = fresh("SC")
        st = lib.rt_scatter_rays_keyed(h, s, ctypes.byref(o), rays_ptr, n,
                                       capi.SC_ALL if outputs is None else outputs,
                                       ctypes.byref(ptrs), ctypes.byref(rec))
        assert st == capi.RT_ERR_INVALID_ARG and untouched(res)
        res, ptrs = fresh("DL")
        st = lib.rt_direct_light_rays_keyed(h, s, ctypes.byref(o), rays_ptr, n,
                                            capi.DL_ALL if outputs is None else outputs,
                                            ctypes.byref(ptrs), ctypes.byref(rec))
        assert st == capi.RT_ERR_INVALID_ARG and untouched(res)
        res, ptrs = fresh("DL")
        st = lib.rt_direct_light_keyed(h, s, ctypes.byref(o), pts.ctypes.data if rays_ptr else None,
                                       mats.ctypes.data, n, n,
                                       capi.DL_ALL if outputs is None else outputs,
                                       ctypes.byref(ptrs), ctypes.byref(rec))
        assert st == capi.RT_ERR_INVALID_ARG and untouched(res)
        if outputs is None:
            T = np.full((n, 5), FILL)
            pn = np.ascontiguousarray(pts[:, :6])
            st = lib.rt_light_transmittance_keyed(h, s, ctypes.byref(o),
                                                  pn.ctypes.data if rays_ptr else None, n,
                                                  T.ctypes.data, ctypes.byref(rec))
            assert st == capi.RT_ERR_INVALID_ARG and (T == FILL).all()
    # the context still answers
    assert_outputs_same(ds.scatter(w["rays"], capi.SC_ALL, area_keys=capi.AreaKeys()),
                        w["got"]["default"]["scatter"], "after the errors")


# ------------------------------------------------------------------ 8. C++ drop-in API
def test_cpp_area_light_scenefile(world, tmp_path):
    """examples/area_light_scenefile --depth 3 on glass_tri_area: the frame composed level by
    level from Scene::ScatterRays with keys leaves no pixel beyond the bar of RenderImage(); --mask
    writes the soft-visibility mask of the first hits."""
    sc = world("glass_tri_area")["sc"]
    scene = tmp_path / "scene.txt"
    sc.write(scene, area_light=True)
    run = subprocess.run([EXE, "--depth", "3", "--mask", str(tmp_path / "mask.pgm"), str(scene)],
                         check=True, capture_output=True, text=True, timeout=120)
    line = next(l for l in run.stdout.splitlines() if l.startswith("depth 3:"))
    words = line.split()
    assert words[words.index("beyond") - 2:words.index("beyond")] == ["0", "pixels"], line
    assert int(words[words.index("of") + 1]) == 384, line
    mask = (tmp_path / "mask.pgm").read_bytes()
    head = b"P5\n24 16\n255\n"
    assert mask.startswith(head) and len(mask) == len(head) + 384
    body = np.frombuffer(mask[len(head):], np.uint8)
    # the same mask from the Python entry: the mean of the area columns of the first hits, 0 on a miss
    ds = world("glass_tri_area")["ds"]
    cam = ds.camera_rays(0)
    idx, pts, _ = shading_points(ds.closest(cam), cam)
    T = ds.light_transmittance(pts[:, :6], area_keys=capi.AreaKeys(idx.astype(np.uint64)))
    al = sc.area_light.samples
    total = np.zeros(len(idx))
    for s in range(al):
        total = total + T[:, len(sc.lights) + s]
    want = np.zeros(384, np.uint8)
    want[idx] = np.floor(total / al * 255.0 + 0.5).astype(np.uint8)
    assert np.array_equal(body, want)
    assert ((body > 0) & (body < 255)).sum() >= 5
