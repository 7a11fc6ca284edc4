"""The transmittance queries (rt_transmittance_rays / rt_light_transmittance and their _device
variants) as far as they go without a device: argument checks, the bindings, the C++ example, and
the register budget of the built gfx950 kernels next to the kernels they share code with."""
import os
import subprocess

import numpy as np
import pytest

from raytracingengine_amd import build, capi
from test_anyhit_host import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rt_transmittance_rays", "rt_transmittance_rays_device",
           "rt_light_transmittance", "rt_light_transmittance_device")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return capi.load_library()


def test_null_arguments_rejected(lib):
    """A NULL context, and NULL input pointers with n > 0, are RT_ERR_INVALID_ARG before anything
    touches a device; the message ends in the entry's name."""
    buf = np.zeros(16, np.float64)
    p = buf.ctypes.data
    for name in ENTRIES:
        fn = getattr(lib, name)
        if "light" in name:
            calls = ((None, None, None, p, 1, p), (None, None, None, None, 1, None))
        else:
            calls = ((None, None, None, p, p, 1, p), (None, None, None, None, None, 1, None))
        for args in calls:
            assert fn(*args) == capi.RT_ERR_INVALID_ARG
            msg = lib.rt_last_error()
            assert b"NULL" in msg and msg.endswith(name.encode()), msg


def test_binding_lists_the_entries():
    assert set(ENTRIES) <= set(capi.EXPORTED)
    for m in ("transmittance", "transmittance_device", "light_transmittance",
              "light_transmittance_device"):
        assert hasattr(capi.DeviceScene, m), m


def test_kernel_source_is_in_the_digest():
    assert "rt_transmit.hip" in build.SOURCES


def test_cpp_example_compiles():
    """examples/transmittance_scenefile.cpp is registered in the build recipe and links against
    the drop-in API, with the batch and the single-ray Scene::ComputeTransmittance resolved by
    librtamd_cpp.so; without arguments it prints its usage."""
    assert build.EXAMPLES.get("transmittance_scenefile") == "transmittance_scenefile.cpp"
    build.build_cpp_api()
    exe = os.path.join(ROOT, "examples", "bin", "transmittance_scenefile")
    assert os.path.exists(exe)
    syms = subprocess.run(["nm", "-C", "-u", exe], capture_output=True, text=True, check=True).stdout
    assert "Scene::ComputeTransmittance(std::vector<Rayon" in syms
    assert "Scene::ComputeTransmittance(Rayon const&, double, double) const" in syms
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 2 and "usage" in run.stderr


def test_register_budget():
    """The BVH stack is the kernels' only private memory — their private segments are no larger
    than intersect_rays_kernel's, so nothing spills — and they hold no more registers than
    trace_rays_kernel<kPathTree, false>, which runs the same march plus the shading."""
    tx = _kernels("rt_transmit.hip")
    rays = {n: r for n, r in tx.items() if "transmittance_rays_kernel" in n}
    light = {n: r for n, r in tx.items() if "light_transmittance_kernel" in n}
    assert len(rays) == 2 and len(light) == 2, sorted(tx)     # OPAQUE false and true of each
    tr = _kernels("rt_trace.hip")
    closest = [r for n, r in tr.items() if "intersect_rays_kernel" in n]
    # trace_rays_kernel<PATH = kPathTree = 2, COUNT = false>: _ZN5rtamd17trace_rays_kernelILi2ELb0EEE...
    tree = [r for n, r in tr.items() if "trace_rays_kernelILi2ELb0EE" in n]
    assert len(closest) == 1 and len(tree) == 1, sorted(tr)
    (_, cpriv), (tregs, tpriv) = closest[0], tree[0]
    print(f"intersect_rays_kernel {cpriv} B private; trace_rays_kernel<tree> {tregs} registers, "
          f"{tpriv} B private")
    for name, (regs, priv) in sorted({**rays, **light}.items()):
        print(f"{name}: {regs} registers, {priv} B private")
        assert priv <= cpriv, name
        assert regs <= tregs, name
