"""The direct-lighting queries (rt_direct_light / rt_direct_light_rays and their _device
variants) as far as they go without a device: argument checks, the bindings, the C++ example, and
the register and private-memory budget of the built gfx950 kernels next to the kernels they
share code with."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from raytracingengine_amd import build, capi
from raytracingengine_amd.scene import Material
from test_anyhit_host import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTS = ("rt_direct_light", "rt_direct_light_device")
RAYS = ("rt_direct_light_rays", "rt_direct_light_rays_device")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return capi.load_library()


def _call(lib, name, inputs=True, outputs=capi.DL_ALL, out="all", n=4, n_materials=4):
    """One call with a NULL context and scene: nothing can reach a device."""
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data
    ptrs = capi.DirectLightPtrs(p, p, p) if out == "all" else out
    ref = ctypes.byref(ptrs) if ptrs is not None else None
    q = p if inputs else None
    if name in POINTS:
        st = getattr(lib, name)(None, None, None, q, q, n_materials, n, outputs, ref)
    else:
        st = getattr(lib, name)(None, None, None, q, n, outputs, ref)
    return st, lib.rt_last_error()


@pytest.mark.parametrize("name", POINTS + RAYS)
def test_bad_arguments_rejected(lib, name):
    """RT_ERR_INVALID_ARG before anything touches a device, each with its own message ending in
    the entry's name: no output bit, an unknown bit, a NULL record, a requested output whose
    pointer is NULL, NULL inputs with n > 0, and a NULL context."""
    p = np.zeros(8, np.float64).ctypes.data
    cases = {
        "no output": dict(outputs=0),
        "unknown output bit": dict(outputs=0x8 | capi.DL_RADIANCE),
        "NULL output record": dict(out=None),
        "NULL pointer of a requested output": dict(outputs=capi.DL_DIFFUSE,
                                                   out=capi.DirectLightPtrs(p, None, p)),
        "NULL argument": dict(inputs=False),
        "NULL context": dict(),
    }
    for text, kw in cases.items():
        st, msg = _call(lib, name, **kw)
        assert st == capi.RT_ERR_INVALID_ARG, (name, text)
        assert text.encode() in msg and msg.endswith(name.encode()), (text, msg)
    # pointers of outputs that were not requested are not looked at: the call gets as far as
    # the context check
    st, msg = _call(lib, name, outputs=capi.DL_SPECULAR, out=capi.DirectLightPtrs(None, None, p))
    assert st == capi.RT_ERR_INVALID_ARG and b"NULL context" in msg


@pytest.mark.parametrize("name", POINTS)
def test_bad_material_count_rejected(lib, name):
    for n_materials in (0, 2, 3, 5):
        st, msg = _call(lib, name, n=4, n_materials=n_materials)
        assert st == capi.RT_ERR_INVALID_ARG
        assert b"n_materials" in msg and msg.endswith(name.encode()), msg
    for n_materials in (1, 4):      # accepted: the call gets as far as the context check
        st, msg = _call(lib, name, n=4, n_materials=n_materials)
        assert st == capi.RT_ERR_INVALID_ARG and b"NULL context" in msg


def test_binding_lists_the_entries():
    assert set(POINTS + RAYS) <= set(capi.EXPORTED)
    for m in ("direct_light", "direct_light_device", "direct_light_rays", "direct_light_rays_device"):
        assert hasattr(capi.DeviceScene, m), m
    assert (capi.DL_RADIANCE, capi.DL_DIFFUSE, capi.DL_SPECULAR, capi.DL_ALL) == (1, 2, 4, 7)
    assert [n for n, _ in capi.DirectLightPtrs._fields_] == ["radiance", "diffuse", "specular"]


def test_material_rows():
    """materials: a Material, seven values, or an [n, 7] array, in rt_material's layout."""
    m = Material((0.1, 0.2, 0.3), shininess=8.0, specular=0.5, transparency=0.25, refractive_index=1.5)
    want = np.array([[0.1, 0.2, 0.3, 8.0, 0.5, 0.25, 1.5]])
    assert np.array_equal(capi.material_rows(m, 5), want)
    assert np.array_equal(capi.material_rows(tuple(want[0]), 5), want)
    assert capi.material_rows(np.tile(want, (5, 1)), 5).shape == (5, 7)
    for bad in (np.zeros((3, 7)), np.zeros(6), np.zeros((5, 8))):
        with pytest.raises(ValueError):
            capi.material_rows(bad, 5)


def test_kernel_source_is_in_the_digest():
    assert "rt_direct.hip" in build.SOURCES


def test_cpp_example_compiles():
    """examples/direct_light_scenefile.cpp is registered in the build recipe and links against the
    drop-in API, with the three Scene::DirectLightning overloads and the host closest hit
    resolved by librtamd_cpp.so; without arguments it prints its usage."""
    assert build.EXAMPLES.get("direct_light_scenefile") == "direct_light_scenefile.cpp"
    build.build_cpp_api()
    exe = os.path.join(ROOT, "examples", "bin", "direct_light_scenefile")
    assert os.path.exists(exe)
    syms = subprocess.run(["nm", "-C", "-u", exe], capture_output=True, text=True, check=True).stdout
    assert "Scene::DirectLightning(HitInfo const&, Vec3 const&, Vec3 const&, double) const" in syms
    assert "Scene::DirectLightning(std::vector<HitInfo" in syms
    assert "Scene::DirectLightning(std::vector<Rayon" in syms
    assert "Scene::IntersectClosestHost(Rayon const&) const" in syms
    for args in ([], ["--host-only"], ["--host-only", "a", "b"]):
        run = subprocess.run([exe, *args], capture_output=True, text=True)
        assert run.returncode == 2 and "usage" in run.stderr


def test_register_budget():
    """The BVH stack is the kernels' only private memory — their private segments are no larger
    than light_transmittance_kernel's, so nothing spills — and they hold no more registers than
    trace_rays_kernel<kPathTree, false>, which runs the same light loop plus the recursion."""
    dk = _kernels("rt_direct.hip")
    points = {n: r for n, r in dk.items() if "direct_light_points_kernel" in n}
    rays = {n: r for n, r in dk.items() if "direct_light_rays_kernel" in n}
    # OPAQUE false and true of each; the points kernel also with and without a shared material
    assert len(points) == 4 and len(rays) == 2, sorted(dk)
    light = [r for n, r in _kernels("rt_transmit.hip").items() if "light_transmittance_kernel" in n]
    # trace_rays_kernel<PATH = kPathTree = 2, COUNT = false>: _ZN5rtamd17trace_rays_kernelILi2ELb0EEE...
    tree = [r for n, r in _kernels("rt_trace.hip").items() if "trace_rays_kernelILi2ELb0EE" in n]
    assert len(light) == 2 and len(tree) == 1
    lpriv = min(priv for _, priv in light)
    tregs = tree[0][0]
    print(f"light_transmittance_kernel {lpriv} B private; trace_rays_kernel<tree> {tregs} registers")
    for name, (regs, priv) in sorted({**points, **rays}.items()):
        print(f"{name}: {regs} registers, {priv} B private")
        assert priv <= lpriv, name
        assert regs <= tregs, name
