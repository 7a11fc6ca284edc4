"""The occlusion query (rt_occluded_rays / rt_occluded_rays_device) as far as it goes without a
device: argument checks, the C++ example, and the register budget of the built gfx950 kernel next
to the closest-hit kernel it is an alternative to."""
import os
import re
import subprocess

import numpy as np
import pytest

from raytracingengine_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "build", "obj")
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return capi.load_library()


def test_null_arguments_rejected(lib):
    """A NULL context, and a NULL rays / max_dist / output pointer with n > 0, are
    RT_ERR_INVALID_ARG before anything touches a device; the message names the entry."""
    buf = np.zeros(16, np.float64)
    p = buf.ctypes.data
    for fn, name in ((lib.rt_occluded_rays, b"rt_occluded_rays"),
                     (lib.rt_occluded_rays_device, b"rt_occluded_rays_device")):
        for args in ((None, None, None, p, p, 1, p), (None, None, None, None, None, 1, None)):
            assert fn(*args) == capi.RT_ERR_INVALID_ARG
            msg = lib.rt_last_error()
            assert b"NULL" in msg and msg.endswith(name), msg


def test_binding_lists_the_entries():
    assert {"rt_occluded_rays", "rt_occluded_rays_device"} <= set(capi.EXPORTED)
    assert hasattr(capi.DeviceScene, "occluded") and hasattr(capi.DeviceScene, "occluded_device")


def _kernels(source):
    """{kernel name: (VGPRs + AGPRs, private segment bytes)} of build/obj/<source>.o."""
    build.build_library()
    obj = os.path.join(OBJ, source + ".o")
    tmp = os.path.join(OBJ, "_meta_" + source)
    os.makedirs(tmp, exist_ok=True)
    fb, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "gfx950.o")
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", obj,
                    os.path.join(tmp, "host.o")], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fb}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True,
                           capture_output=True, text=True).stdout
    out = {}
    for entry in re.split(r"\n  - \.", notes):  # kernel records (argument records are deeper)
        name = re.search(r"\n    \.name:\s+(\S+)", entry)
        v = re.search(r"vgpr_count:\s+(\d+)", entry)
        a = re.search(r"^agpr_count:\s+(\d+)", entry)
        s = re.search(r"private_segment_fixed_size:\s+(\d+)", entry)
        if name and v and a and s and "_kernel" in name.group(1):
            out[name.group(1)] = (int(v.group(1)) + int(a.group(1)), int(s.group(1)))
    return out


def test_register_budget_against_closest_hit():
    """occluded_rays_kernel carries the BVH stack intersect_rays_kernel carries and less state
    (no best t, kind, index, normal or hit point): its registers and its private segment are no
    larger than that kernel's in the same build."""
    any_hit = {n: r for n, r in _kernels("rt_anyhit.hip").items() if "occluded_rays_kernel" in n}
    closest = {n: r for n, r in _kernels("rt_trace.hip").items() if "intersect_rays_kernel" in n}
    assert len(any_hit) == 1 and len(closest) == 1, (sorted(any_hit), sorted(closest))
    (regs, priv), (cregs, cpriv) = list(any_hit.values())[0], list(closest.values())[0]
    print(f"occluded_rays_kernel {regs} registers, {priv} B private; "
          f"intersect_rays_kernel {cregs} registers, {cpriv} B private")
    assert regs <= cregs and priv <= cpriv


def test_cpp_example_compiles():
    """examples/occlusion_scenefile.cpp is registered in the build recipe and links against the
    drop-in API, with the batch Scene::IntersectAnyBefore resolved by librtamd_cpp.so."""
    assert build.EXAMPLES.get("occlusion_scenefile") == "occlusion_scenefile.cpp"
    build.build_cpp_api()
    exe = os.path.join(ROOT, "examples", "bin", "occlusion_scenefile")
    assert os.path.exists(exe)
    syms = subprocess.run(["nm", "-C", "-u", exe], capture_output=True, text=True, check=True).stdout
    assert "Scene::IntersectAnyBefore(std::vector<Rayon" in syms
    assert "Scene::IntersectAnyBefore(Rayon const&, double) const" in syms
    assert subprocess.run([exe], capture_output=True).returncode == 2  # usage
