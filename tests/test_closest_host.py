"""The camera-ray, closest-hit and device TraceRay queries (rt_camera_rays[_device],
rt_closest_rays[_device], rt_trace_rays_device) as far as they go without a device: argument
checks, the bindings, the build recipe, the C++ example, and the register and private-memory
budget of the built gfx950 kernels next to intersect_rays_kernel, the parent's closest hit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from raytracingengine_amd import build, capi
from raytracingengine_amd.scene import CAMERA_DTYPE
from test_anyhit_host import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOSEST = ("rt_closest_rays", "rt_closest_rays_device")
CAMERA = ("rt_camera_rays", "rt_camera_rays_device")
ENTRIES = CLOSEST + CAMERA + ("rt_trace_rays_device",)
FIELDS = ["t", "prim", "normal", "point", "material"]


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return capi.load_library()


def _closest(lib, name, inputs=True, outputs=capi.CH_ALL, out="all", n=4):
    """One call with a NULL context and scene: nothing can reach a device."""
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data
    ptrs = capi.ClosestPtrs(p, p, p, p, p) if out == "all" else out
    ref = ctypes.byref(ptrs) if ptrs is not None else None
    st = getattr(lib, name)(None, None, None, p if inputs else None, n, outputs, ref)
    return st, lib.rt_last_error()


def _camera(width=24, height=16, aa=4):
    cam = np.zeros(1, CAMERA_DTYPE)
    cam["position"][0] = (0.0, 0.0, -25.0)
    cam["focal"] = 12.0
    cam["width"], cam["height"], cam["aa_samples"] = width, height, aa
    return cam


@pytest.mark.parametrize("name", CLOSEST)
def test_closest_bad_arguments_rejected(lib, name):
    """RT_ERR_INVALID_ARG before anything touches a device, rt_scatter_rays' cases with its
    message texts, each ending in the entry's name: no output bit, an unknown bit, a NULL record,
    a requested output whose pointer is NULL, NULL rays with n > 0, and a NULL context."""
    p = np.zeros(8, np.float64).ctypes.data
    cases = {
        "no output": dict(outputs=0),
        "unknown output bit": dict(outputs=0x20 | capi.CH_T),
        "NULL output record": dict(out=None),
        "NULL pointer of a requested output": dict(outputs=capi.CH_POINT,
                                                   out=capi.ClosestPtrs(p, p, p, None, p)),
        "NULL argument": dict(inputs=False),
        "NULL context": dict(),
    }
    for text, kw in cases.items():
        st, msg = _closest(lib, name, **kw)
        assert st == capi.RT_ERR_INVALID_ARG, (name, text)
        assert text.encode() in msg and msg.endswith(name.encode()), (text, msg)
    for bit, field in zip((1, 2, 4, 8, 16), FIELDS):
        ptrs = capi.ClosestPtrs(p, p, p, p, p)
        setattr(ptrs, field, None)
        st, msg = _closest(lib, name, outputs=bit, out=ptrs)
        assert st == capi.RT_ERR_INVALID_ARG and b"NULL pointer of a requested output" in msg, field
        # pointers of outputs that were not requested are not looked at: the call gets as far as
        # the context check
        st, msg = _closest(lib, name, outputs=capi.CH_ALL & ~bit, out=ptrs)
        assert st == capi.RT_ERR_INVALID_ARG and b"NULL context" in msg, field
    # n == 0 with NULL rays passes the argument checks and stops at the context
    st, msg = _closest(lib, name, inputs=False, n=0)
    assert st == capi.RT_ERR_INVALID_ARG and b"NULL context" in msg


@pytest.mark.parametrize("name", CAMERA)
def test_camera_bad_arguments_rejected(lib, name):
    """A NULL context, camera or output; a zero-size camera; a sample outside
    [0, max(1, aa_samples)).  The checks come before the context is used: a context that is only
    a non-NULL address is never dereferenced by a rejected call."""
    fn = getattr(lib, name)
    buf = np.zeros(8, np.float64)
    p, cam = buf.ctypes.data, _camera()
    fake_ctx = buf.ctypes.data   # never reached: every call below fails an earlier check
    for args in ((None, cam.ctypes.data, None, 0, p), (fake_ctx, None, None, 0, p),
                 (fake_ctx, cam.ctypes.data, None, 0, None)):
        assert fn(*args) == capi.RT_ERR_INVALID_ARG
        msg = lib.rt_last_error()
        assert b"NULL" in msg and msg.endswith(name.encode()), msg
    for w, h in ((0, 16), (24, 0), (0, 0)):
        assert fn(fake_ctx, _camera(w, h).ctypes.data, None, 0, p) == capi.RT_ERR_INVALID_ARG
        msg = lib.rt_last_error()
        assert b"width or height" in msg and msg.endswith(name.encode()), msg
    for aa, sample in ((4, -1), (4, 4), (4, 100), (1, 1), (0, 1), (-3, 1)):
        st = fn(fake_ctx, _camera(aa=aa).ctypes.data, None, sample, p)
        assert st == capi.RT_ERR_INVALID_ARG, (aa, sample)
        msg = lib.rt_last_error()
        assert b"sample" in msg and msg.endswith(name.encode()), msg
    # a row set outside the image
    o = capi.default_opts(row_begin=16)
    assert fn(fake_ctx, cam.ctypes.data, ctypes.byref(o), 0, p) == capi.RT_ERR_INVALID_ARG
    assert b"row range" in lib.rt_last_error()


def test_trace_rays_device_null_arguments(lib):
    p = np.zeros(8, np.float64).ctypes.data
    for args in ((None, None, None, p, 4, p), (None, None, None, None, 0, None)):
        assert lib.rt_trace_rays_device(*args) == capi.RT_ERR_INVALID_ARG
        msg = lib.rt_last_error()
        assert b"NULL" in msg and msg.endswith(b"rt_trace_rays_device"), msg


def test_binding_lists_the_entries():
    assert set(ENTRIES) <= set(capi.EXPORTED)
    for m in ("camera_rays", "camera_rays_device", "closest", "closest_device",
              "trace_rays_device"):
        assert hasattr(capi.DeviceScene, m), m
    assert (capi.CH_T, capi.CH_PRIM, capi.CH_NORMAL, capi.CH_POINT, capi.CH_MATERIAL,
            capi.CH_ALL) == (1, 2, 4, 8, 16, 31)
    assert [n for n, _ in capi.ClosestPtrs._fields_] == FIELDS
    assert [(n, np.dtype(dt), k) for n, _, dt, k in capi.CH_OUTPUTS] == [
        ("t", np.float64, 0), ("prim", np.int32, 2), ("normal", np.float64, 3),
        ("point", np.float64, 3), ("material", np.float64, 7)]
    with open(os.path.join(ROOT, "include", "rt_capi.h")) as fh:
        header = fh.read()
    for name, value in (("RT_CH_T", 1), ("RT_CH_PRIM", 2), ("RT_CH_NORMAL", 4),
                        ("RT_CH_POINT", 8), ("RT_CH_MATERIAL", 16), ("RT_CH_ALL", 31)):
        line = next(l for l in header.splitlines() if l.startswith(f"#define {name} "))
        assert int(line.split()[2], 16) == value, line
    # the record's members in the header, in the binding's order
    body = header.split("struct rt_closest_out {")[1].split("}")[0]
    assert [l.split()[1].rstrip(";") for l in body.strip().splitlines()] == FIELDS
    for bad in (0, 0x20, 0x3f):
        with pytest.raises(ValueError):
            capi._ch_check(bad)


def test_kernel_sources_are_in_the_digest():
    for src in ("rt_camera_rays.hip", "rt_closest.hip"):
        assert src in build.SOURCES
        assert os.path.exists(os.path.join(build.CSRC, src))
    assert len(build.source_digest()) == 64


def test_cpp_example_compiles():
    """examples/closest_scenefile.cpp is registered in the build recipe and links against the
    drop-in API, with Scene::CameraRays and the batch Scene::IntersectClosest resolved by
    librtamd_cpp.so; with the wrong number of arguments it prints its usage."""
    assert build.EXAMPLES.get("closest_scenefile") == "closest_scenefile.cpp"
    build.build_cpp_api()
    exe = os.path.join(ROOT, "examples", "bin", "closest_scenefile")
    assert os.path.exists(exe)
    syms = subprocess.run(["nm", "-C", "-u", exe], capture_output=True, text=True, check=True).stdout
    assert "Scene::IntersectClosest(std::vector<Rayon" in syms
    assert "Scene::CameraRays(int) const" in syms
    for args in ([], ["--camera", "1"], ["--camera", "1", "a", "b", "c"], ["a", "b"]):
        run = subprocess.run([exe, *args], capture_output=True, text=True)
        assert run.returncode == 2 and "usage" in run.stderr


def test_register_budget():
    """No closest kernel holds more VGPRs + AGPRs than intersect_rays_kernel (rt_trace.hip), the
    parent's kernel for the same work; the T | PRIM instantiation (FULL = false) holds no more
    than the CH_ALL one; and no new kernel has a private segment: the closest kernels keep the
    BVH traversal stack in LDS, the camera-ray kernel has nothing to keep."""
    ck = {n: r for n, r in _kernels("rt_closest.hip").items() if "closest_rays_kernel" in n}
    cam = {n: r for n, r in _kernels("rt_camera_rays.hip").items() if "camera_rays_kernel" in n}
    parent = [r for n, r in _kernels("rt_trace.hip").items() if "intersect_rays_kernel" in n]
    assert len(ck) == 2 and len(cam) == 1 and len(parent) == 1, (sorted(ck), sorted(cam))
    pregs, ppriv = parent[0]
    print(f"intersect_rays_kernel: {pregs} registers, {ppriv} B private")
    for name, (regs, priv) in sorted({**ck, **cam}.items()):
        print(f"{name}: {regs} registers, {priv} B private")
        assert priv == 0, name
    for name, (regs, _) in ck.items():
        assert regs <= pregs, name
    # closest_rays_kernel<FULL>: ...closest_rays_kernelILb0EE... is T | PRIM, ILb1EE the rest
    lean = next(r for n, r in ck.items() if "closest_rays_kernelILb0EE" in n)
    full = next(r for n, r in ck.items() if "closest_rays_kernelILb1EE" in n)
    assert lean[0] <= full[0]
