"""Progressive frames (rt_accumulate_samples[_device], rt_resolve[_device], rt_accumulate.hip) as
far as they go without a device: argument checks, the bindings, the build recipe, the default
schedule, the C++ example, and the register and private-memory budget of the built gfx950 kernels
next to trace_rays_kernel, the kernel of the unfused composition."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from raytracingengine_amd import build, capi
from raytracingengine_amd.scene import CAMERA_DTYPE
from test_anyhit_host import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCUMULATE = ("rt_accumulate_samples", "rt_accumulate_samples_device")
RESOLVE = ("rt_resolve", "rt_resolve_device")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return capi.load_library()


def _camera(width=24, height=16, aa=4):
    cam = np.zeros(1, CAMERA_DTYPE)
    cam["position"][0] = (0.0, 0.0, -25.0)
    cam["focal"] = 12.0
    cam["width"], cam["height"], cam["aa_samples"] = width, height, aa
    return cam


def _rejected(lib, name, args, text):
    assert getattr(lib, name)(*args) == capi.RT_ERR_INVALID_ARG, (name, text, args)
    msg = lib.rt_last_error()
    assert text.encode() in msg and msg.endswith(name.encode()), (name, text, msg)


@pytest.mark.parametrize("name", ACCUMULATE)
def test_accumulate_bad_arguments_rejected(lib, name):
    """RT_ERR_INVALID_ARG before anything touches a device, the message ending in the entry's
    name: a NULL context, scene, camera or sum; a zero-size camera; sample_begin < 0, sample_begin
    >= sample_end, sample_end > max(1, aa_samples); a row set outside the image.  Every case is
    made with a NULL context, with a NULL scene, and with both only non-NULL addresses: the
    checks come before either is dereferenced."""
    buf = np.zeros(8, np.float64)
    p, fake = buf.ctypes.data, buf.ctypes.data   # `fake` is never reached by a rejected call
    cam = _camera().ctypes.data
    for args in ((None, fake, cam, None, 0, 1, p), (fake, None, cam, None, 0, 1, p),
                 (fake, fake, None, None, 0, 1, p), (fake, fake, cam, None, 0, 1, None),
                 (None, None, None, None, 0, 1, None)):
        _rejected(lib, name, args, "NULL")
    for ctx, scene in ((fake, fake), (None, fake), (fake, None), (None, None)):
        text = (lambda t: t) if ctx and scene else (lambda t: "NULL")
        for w, h in ((0, 16), (24, 0), (0, 0)):
            _rejected(lib, name, (ctx, scene, _camera(w, h).ctypes.data, None, 0, 1, p),
                      text("width or height"))
        for aa, s0, s1 in ((4, -1, 2), (4, 2, 2), (4, 3, 1), (4, 0, 5), (4, 4, 5), (4, 0, 100),
                           (1, 0, 2), (1, 1, 2), (0, 0, 2), (-3, 0, 2), (4, 0, 0)):
            _rejected(lib, name, (ctx, scene, _camera(aa=aa).ctypes.data, None, s0, s1, p),
                      text("sample range"))
        for kw, what in ((dict(row_begin=16), "row range"), (dict(row_end=17), "row range"),
                         (dict(row_begin=5, row_end=5), "row range"),
                         (dict(row_cycle=3, row_block=0), "row_cycle")):
            o = capi.default_opts(**kw)
            _rejected(lib, name, (ctx, scene, cam, ctypes.byref(o), 0, 4, p), text(what))


@pytest.mark.parametrize("name", RESOLVE)
def test_resolve_bad_arguments_rejected(lib, name):
    """samples < 1, an unknown operator, no output, bytes with RT_TONEMAP_NONE, a NULL sum with
    n > 0 and a NULL context, in that order, each before the context is dereferenced; n == 0
    with valid arguments returns RT_OK without reaching a device."""
    buf = np.zeros(64, np.float64)
    p, fake = buf.ctypes.data, buf.ctypes.data
    for ctx in (fake, None):
        for samples in (0, -1, -100):
            _rejected(lib, name, (ctx, p, 4, samples, capi.TONEMAP_NONE, p, None, None), "samples")
        for op in (-2, 8, 100):
            _rejected(lib, name, (ctx, p, 4, 1, op, p, None, p), "tonemap")
        for op in (capi.TONEMAP_NONE, 1, capi.TONEMAP_ALL):
            _rejected(lib, name, (ctx, p, 4, 1, op, None, None, None), "no output")
        _rejected(lib, name, (ctx, p, 4, 1, capi.TONEMAP_NONE, p, None, p), "RT_TONEMAP_NONE")
        _rejected(lib, name, (ctx, p, 4, 1, capi.TONEMAP_NONE, None, None, p), "RT_TONEMAP_NONE")
        _rejected(lib, name, (ctx, None, 4, 1, 1, p, p, p), "NULL sum")
    _rejected(lib, name, (None, p, 4, 1, 1, p, p, p), "NULL context")
    _rejected(lib, name, (None, None, 0, 1, 1, p, p, p), "NULL context")
    for args in ((fake, None, 0, 1, 1, p, p, p), (fake, p, 0, 3, capi.TONEMAP_ALL, None, None, p),
                 (fake, None, 0, 1, capi.TONEMAP_NONE, None, p, None)):
        assert getattr(lib, name)(*args) == capi.RT_OK, args


def test_binding_lists_the_entries():
    assert set(ACCUMULATE + RESOLVE) <= set(capi.EXPORTED)
    for m in ("accumulate", "accumulate_device", "resolve", "resolve_device", "render_progressive"):
        assert hasattr(capi.DeviceScene, m), m
    with open(os.path.join(ROOT, "include", "rt_capi.h")) as fh:
        header = fh.read()
    for name in ACCUMULATE + RESOLVE:
        assert re.search(rf"\nrt_status {name}\(", header), name
    assert "Scene.h:283-304" in header.split("rt_status rt_accumulate_samples_device(")[0][-4000:]


def test_progressive_schedule():
    assert capi.progressive_schedule(1) == [1]
    assert capi.progressive_schedule(4) == [1, 2, 4]
    assert capi.progressive_schedule(6) == [1, 2, 4, 6]
    assert capi.progressive_schedule(32) == [1, 2, 4, 8, 16, 32]
    # a camera without anti-aliasing has the one sample GeneratePixelAt gives it
    assert capi.progressive_schedule(0) == [1] and capi.progressive_schedule(-2) == [1]
    assert capi.progressive_schedule(2) == [1, 2] and capi.progressive_schedule(3) == [1, 2, 3]
    for aa in range(1, 70):
        s = capi.progressive_schedule(aa)
        assert s[0] == 1 and s[-1] == aa and all(b > a for a, b in zip(s, s[1:])), aa


def test_kernel_source_is_in_the_recipe_and_the_digest():
    assert "rt_accumulate.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "rt_accumulate.hip"))
    assert len(build.source_digest()) == 64
    with open(os.path.join(build.CSRC, "rt_internal.hpp")) as fh:
        internal = fh.read()
    assert "launch_accumulate_samples(" in internal and "launch_resolve(" in internal


def test_register_and_private_memory_budget():
    """accumulate_samples_kernel<PATH>, one per TraceRay shape: at least 2 waves per SIMD (at most
    256 VGPRs + AGPRs, the budget test_kernel_occupancy.py holds the generic trace kernels to) and
    no more private memory per lane than trace_rays_kernel<PATH, COUNT = false> of the same build —
    the sample loop and the resident sum cost the composition's kernel no spill.  resolve_kernel
    has no private segment."""
    acc = {n: r for n, r in _kernels("rt_accumulate.hip").items() if "accumulate_samples_kernel" in n}
    res = [r for n, r in _kernels("rt_accumulate.hip").items() if "resolve_kernel" in n]
    rays = {n: r for n, r in _kernels("rt_trace.hip").items() if "trace_rays_kernel" in n}
    assert len(acc) == 3 and len(res) == 1 and len(rays) == 6, (sorted(acc), sorted(rays))
    for path in (0, 1, 2):
        name, (regs, priv) = next((n, r) for n, r in acc.items()
                                  if f"accumulate_samples_kernelILi{path}EE" in n)
        pregs, ppriv = next(r for n, r in rays.items() if f"trace_rays_kernelILi{path}ELb0EE" in n)
        print(f"path {path}: accumulate_samples_kernel {regs} registers, {priv} B private; "
              f"trace_rays_kernel {pregs} registers, {ppriv} B private")
        alloc = max(8, -(-regs // 8) * 8)
        assert min(8, 512 // alloc) >= 2, (name, regs)
        assert priv <= ppriv, (name, priv, ppriv)
    print(f"resolve_kernel: {res[0][0]} registers, {res[0][1]} B private")
    assert res[0][1] == 0


def test_cpp_example_compiles():
    """examples/progressive_scenefile.cpp is registered in the build recipe and links against the
    drop-in API, with Scene::AccumulateSamples and rtamd::resolve resolved by librtamd_cpp.so;
    with the wrong number of arguments it prints its usage."""
    assert build.EXAMPLES.get("progressive_scenefile") == "progressive_scenefile.cpp"
    build.build_cpp_api()
    exe = os.path.join(ROOT, "examples", "bin", "progressive_scenefile")
    assert os.path.exists(exe)
    syms = subprocess.run(["nm", "-C", "-u", exe], capture_output=True, text=True, check=True).stdout
    assert "Scene::AccumulateSamples(int, int, std::vector<Vec3" in syms
    assert "rtamd::resolve(std::vector<Vec3" in syms
    assert "rtamd::resolveTonemapped(std::vector<Vec3" in syms
    for args in ([], ["--check"], ["--check", "a"], ["a", "b", "c"]):
        run = subprocess.run([exe, *args], capture_output=True, text=True)
        assert run.returncode == 2 and "usage" in run.stderr
