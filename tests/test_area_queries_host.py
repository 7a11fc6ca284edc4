"""The keyed queries (rt_scatter_rays_keyed, rt_direct_light_keyed, rt_direct_light_rays_keyed,
rt_light_transmittance_keyed and their _device twins) as far as they go without a device: the
numpy restatement the GPU tests compare with (tests/area_query_sets.py) is held to the oracle's
TraceRay and RenderImage on the two area-light scenes, then the argument checks, the bindings and
the register budget of the built gfx950 kernels."""
import ctypes

import numpy as np
import pytest

import area_query_sets as aq
import raysets
from oracle import pyoracle as po
from raytracingengine_amd import build, capi
from raytracingengine_amd.configs import make_config
from test_anyhit_host import _kernels

SC, DL, LT = "scatter", "direct", "light"
# entry -> the shape of its arguments
ENTRIES = {
    "rt_scatter_rays_keyed": SC, "rt_scatter_rays_keyed_device": SC,
    "rt_direct_light_rays_keyed": DL, "rt_direct_light_rays_keyed_device": DL,
    "rt_direct_light_keyed": "points", "rt_direct_light_keyed_device": "points",
    "rt_light_transmittance_keyed": LT, "rt_light_transmittance_keyed_device": LT,
}
KERNELS = ("keyed_scatter_kernel", "keyed_direct_points_kernel", "keyed_direct_rays_kernel",
           "keyed_shadow_points_kernel")
# the un-keyed kernels' names, by which the other host tests select them
TAKEN = ("scatter_rays_kernel", "direct_light_points_kernel", "direct_light_rays_kernel",
         "light_transmittance_kernel")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return capi.load_library()


# ---------------------------------------------------------------- the restatement is the oracle's
def test_level_is_the_oracle_on_c5():
    """c5's 648 rays with pixel = i, sample 0, depth 0: the keyed level's value is TraceRay with
    max_recursion = 1, bit for bit; the scene is opaque with no specular above the bias, so no
    level has a child."""
    t = aq.table("c5", "default")
    ref, _, _ = po.trace_rays(t["sc"], t["rays"], max_recursion=1)
    off, _, _ = po.trace_rays(t["sc"], t["rays"], max_recursion=1, use_area_light=False)
    lv = t["scatter"]
    hit = (lv["flags"] & 1) != 0
    matters = int((ref != off).any(axis=1).sum())
    print(f"c5: {hit.sum()} hits, {(~hit).sum()} misses, {matters} rays change with the area light")
    assert hit.sum() >= 100 and (~hit).sum() >= 100 and matters >= 50
    assert not (lv["flags"] & 6).any()
    assert not lv["pow_value"].any()
    assert aq.same_bits(lv["value"], ref)


@pytest.fixture(scope="module")
def glass():
    sc = raysets.scene("glass_tri_area")
    rays, _ = raysets.rayset(sc)
    return sc, rays


def test_composition_is_the_oracle(glass):
    sc, rays = glass
    ref, _, _ = po.trace_rays(sc, rays, max_recursion=3)
    off, _, _ = po.trace_rays(sc, rays, max_recursion=3, use_area_light=False)
    matters = int((ref != off).any(axis=1).sum())
    print(f"glass_tri_area: {matters} of {len(rays)} rays change with the area light")
    assert matters >= 300
    got = aq.compose(sc, rays, 3)
    assert aq.within_bar(got, ref).all(), np.abs(got - ref).max()


def test_depth_key_matters(glass):
    """The same composition with depth = 0 at every level draws the children's samples from the
    first level's stream: it is not the oracle's TraceRay."""
    sc, rays = glass
    ref, _, _ = po.trace_rays(sc, rays, max_recursion=3)
    got = aq.compose(sc, rays, 3, depth_key=lambda level: 0)
    differ = int((~aq.within_bar(got, ref)).any(axis=1).sum())
    print(f"depth = 0 at every level: {differ} rays leave the bar")
    assert differ >= 1


def test_composition_is_the_frame(glass):
    sc, _ = glass
    ref, _, _ = po.render(sc, max_recursion=3)
    off, _, _ = po.render(sc, max_recursion=3, use_area_light=False)
    matters = int((ref != off).any(axis=2).sum())
    print(f"glass_tri_area: {matters} of {ref.shape[0] * ref.shape[1]} pixels change")
    assert matters >= 192
    got = aq.compose(sc, raysets.camera_rays(sc), 3, pixel=aq.frame_pixels(sc))
    assert aq.within_bar(got.reshape(ref.shape), ref).all()


def test_frame_from_its_samples():
    """c5 at 24x16 with four AA samples: ((0 + v_0) + v_1 + v_2 + v_3) / 4 with v_s the level's
    value on the sample's camera rays under the keys (y*W + x, s, 0) is RenderImage, bit for bit."""
    sc = make_config("c5", 24, 16, aa=4)
    w, h = sc.camera.width, sc.camera.height
    ref, _, _ = po.render(sc)
    off, _, _ = po.render(sc, use_area_light=False)
    assert int((ref != off).any(axis=2).sum()) >= 20
    total = np.zeros((w * h, 3), np.float64)
    for s in range(4):
        rays = np.array([po.get_ray(sc, x, y, aa=s > 0, seed=aq.SEED, sample=s)
                         for y in range(h) for x in range(w)])
        total = total + aq.level(sc, rays, aq.frame_pixels(sc), sample=s)["value"]
    assert aq.same_bits((total / 4.0).reshape(ref.shape), ref)


# ---------------------------------------------------------------- argument checks, no device
def _call(lib, name, ctx=None, keys=(None, 0, 0), outputs=None, n=4):
    """One call without a scene: nothing can reach a device."""
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data
    rec = capi.AreaKeysRec(*keys)
    kref = ctypes.byref(rec)
    fam = ENTRIES[name]
    fn = getattr(lib, name)
    if fam == LT:
        st = fn(ctx, None, None, p, n, p, kref)
    elif fam == SC:
        ptrs = capi.ScatterPtrs(p, p, p, p, p)
        st = fn(ctx, None, None, p, n, capi.SC_ALL if outputs is None else outputs,
                ctypes.byref(ptrs), kref)
    else:
        ptrs = capi.DirectLightPtrs(p, p, p)
        o = capi.DL_ALL if outputs is None else outputs
        if fam == "points":
            st = fn(ctx, None, None, p, p, 1, n, o, ctypes.byref(ptrs), kref)
        else:
            st = fn(ctx, None, None, p, n, o, ctypes.byref(ptrs), kref)
    return st, lib.rt_last_error()


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_bad_arguments_rejected(lib, name):
    """RT_ERR_INVALID_ARG before anything touches a device, the message ending in the entry's
    name: a NULL context, depth = 64, sample = 0x01000000 and, where the entry has them,
    outputs = 0.  The largest valid keys pass the key checks and stop at the context."""
    cases = {"NULL": dict(), "depth": dict(keys=(None, 0, 64)),
             "sample": dict(keys=(None, 0x01000000, 0))}
    if ENTRIES[name] != LT:
        cases["no output"] = dict(outputs=0)
    for text, kw in cases.items():
        st, msg = _call(lib, name, **kw)
        assert st == capi.RT_ERR_INVALID_ARG, (name, text)
        assert text.encode() in msg and msg.endswith(name.encode()), (text, msg)
    st, msg = _call(lib, name, keys=(None, 0x00FFFFFF, 63))
    assert st == capi.RT_ERR_INVALID_ARG and b"NULL" in msg, msg


def test_binding_lists_the_entries():
    assert set(ENTRIES) <= set(capi.EXPORTED)
    import inspect
    for m in ("scatter", "direct_light", "direct_light_rays", "light_transmittance"):
        for meth in (m, m + "_device"):
            sig = inspect.signature(getattr(capi.DeviceScene, meth))
            assert sig.parameters["area_keys"].default is None, meth
            assert "seed" in sig.parameters, meth
    assert inspect.signature(capi.compose_trace).parameters["area_keys"].default is None
    k = capi.AreaKeys()
    assert (k.pixel, k.sample, k.depth) == (None, 0, 0)
    assert ctypes.sizeof(capi.AreaKeysRec) == 16
    with pytest.raises(ValueError):
        capi.AreaKeys(pixel=[1, 2, 3])._host(4)


def test_kernels_and_register_budget():
    """The keyed kernels stand next to their un-keyed siblings, in the objects of rt_scatter.hip,
    rt_direct.hip and rt_transmit.hip, under names the other host tests' selections do not match,
    each within 256 VGPRs + AGPRs: two waves per SIMD, the rule tests/test_kernel_occupancy.py
    applies to the generic trace kernels."""
    sources = ("rt_scatter.hip", "rt_direct.hip", "rt_direct.hip", "rt_transmit.hip")
    keyed = {}
    for want, source, count in zip(KERNELS, sources, (4, 4, 2, 2)):
        assert source in build.SOURCES
        ks = _kernels(source)
        got = {n: r for n, r in ks.items() if want in n}
        assert len(got) == count, (want, sorted(ks))
        for name, (regs, priv) in sorted(got.items()):
            print(f"{name}: {regs} registers, {priv} B private")
            assert regs <= 256, name
        keyed.update(got)
    for name in keyed:
        assert not any(t in name for t in TAKEN), name
