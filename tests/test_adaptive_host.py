"""Adaptive progressive frames (rt_accumulate_adaptive[_device], rt_resolve_counts[_device],
rt_adaptive.hip) as far as they go without a device: argument checks, the bindings, the build
recipe, the register and private-memory budget of the built gfx950 kernels next to
accumulate_samples_kernel, the C++ example, and the stop rule's numpy form on the C oracle's
per-sample colours."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_sets
from adaptive_sets import AA, FRAMES, RULE, SEED, stop_counts
from raytracingengine_amd import build, capi
from raytracingengine_amd.configs import make_config
from raytracingengine_amd.scene import CAMERA_DTYPE
from test_anyhit_host import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAPTIVE = ("rt_accumulate_adaptive", "rt_accumulate_adaptive_device")
RESOLVE = ("rt_resolve_counts", "rt_resolve_counts_device")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return capi.load_library()


def _camera(width=24, height=16, aa=8):
    cam = np.zeros(1, CAMERA_DTYPE)
    cam["position"][0] = (0.0, 0.0, -25.0)
    cam["focal"] = 12.0
    cam["width"], cam["height"], cam["aa_samples"] = width, height, aa
    return cam


def _rule(tolerance=0.05, lum_floor=0.01, min_samples=2):
    return capi.AdaptiveRule(tolerance, lum_floor, min_samples, 0)


def _rejected(lib, name, args, text):
    assert getattr(lib, name)(*args) == capi.RT_ERR_INVALID_ARG, (name, text, args)
    msg = lib.rt_last_error()
    assert text.encode() in msg and msg.endswith(name.encode()), (name, text, msg)


@pytest.mark.parametrize("name", ADAPTIVE)
def test_adaptive_bad_arguments_rejected(lib, name):
    """RT_ERR_INVALID_ARG before anything is dereferenced or a device is touched, the message
    ending in the entry's name: a NULL context, scene, camera, rule or array; a zero-size camera;
    sample_end < 1 or > max(1, aa_samples); min_samples < 2; a negative or NaN tolerance; a
    lum_floor not above 0; a row set outside the image.  Every case after the NULL ones is made
    with a NULL context, a NULL scene, and with both only non-NULL addresses."""
    buf = np.zeros(8, np.float64)
    p, fake = buf.ctypes.data, buf.ctypes.data   # `fake` is never reached by a rejected call
    keep = []                    # the camera records stay alive while the calls read them

    def cam_at(*a, **kw):
        keep.append(_camera(*a, **kw))
        return keep[-1].ctypes.data
    cam = cam_at()
    ok = _rule()
    r = ctypes.addressof(ok)
    for args in ((None, fake, cam, None, r, 1, 1, p, p, p), (fake, None, cam, None, r, 1, 1, p, p, p),
                 (fake, fake, None, None, r, 1, 1, p, p, p), (fake, fake, cam, None, None, 1, 1, p, p, p),
                 (fake, fake, cam, None, r, 1, 1, None, p, p), (fake, fake, cam, None, r, 1, 1, p, None, p),
                 (fake, fake, cam, None, r, 1, 1, p, p, None),
                 (None, None, None, None, None, 0, 1, None, None, None)):
        _rejected(lib, name, args, "NULL")
    for ctx, scene in ((fake, fake), (None, fake), (fake, None), (None, None)):
        text = (lambda t: t) if ctx and scene else (lambda t: "NULL")
        for fresh in (0, 1):
            for w, h in ((0, 16), (24, 0), (0, 0)):
                _rejected(lib, name, (ctx, scene, cam_at(w, h), None, r, fresh, 1, p, p, p),
                          text("width or height"))
            for aa, end in ((8, 0), (8, -1), (8, 9), (8, 100), (1, 2), (0, 2), (-3, 2)):
                _rejected(lib, name, (ctx, scene, cam_at(aa=aa), None, r, fresh, end, p, p, p),
                          text("sample_end"))
            for bad, what in ((_rule(min_samples=1), "min_samples"), (_rule(min_samples=0), "min_samples"),
                              (_rule(min_samples=-5), "min_samples"),
                              (_rule(tolerance=-1e-300), "tolerance"),
                              (_rule(tolerance=float("nan")), "tolerance"),
                              (_rule(tolerance=-float("inf")), "tolerance"),
                              (_rule(lum_floor=0.0), "lum_floor"), (_rule(lum_floor=-0.0), "lum_floor"),
                              (_rule(lum_floor=-1.0), "lum_floor"),
                              (_rule(lum_floor=float("nan")), "lum_floor")):
                _rejected(lib, name, (ctx, scene, cam, None, ctypes.addressof(bad), fresh, 4, p, p, p),
                          text(what))
            for kw, what in ((dict(row_begin=16), "row range"), (dict(row_end=17), "row range"),
                             (dict(row_begin=5, row_end=5), "row range"),
                             (dict(row_cycle=3, row_block=0), "row_cycle")):
                o = capi.default_opts(**kw)
                _rejected(lib, name, (ctx, scene, cam, ctypes.byref(o), r, fresh, 4, p, p, p), text(what))


@pytest.mark.parametrize("name", RESOLVE)
def test_resolve_counts_bad_arguments_rejected(lib, name):
    """rt_resolve's checks in its order (an unknown operator, no output, bytes with
    RT_TONEMAP_NONE, a NULL sum with n > 0), then a NULL count with n > 0, then a NULL context,
    each before the context is dereferenced; n == 0 with valid arguments returns RT_OK without
    reaching a device."""
    buf = np.zeros(64, np.float64)
    p, fake = buf.ctypes.data, buf.ctypes.data
    for ctx in (fake, None):
        for op in (-2, 8, 100):
            _rejected(lib, name, (ctx, p, p, 4, op, p, None, p), "tonemap")
        for op in (capi.TONEMAP_NONE, 1, capi.TONEMAP_ALL):
            _rejected(lib, name, (ctx, p, p, 4, op, None, None, None), "no output")
        _rejected(lib, name, (ctx, p, p, 4, capi.TONEMAP_NONE, p, None, p), "RT_TONEMAP_NONE")
        _rejected(lib, name, (ctx, None, p, 4, 1, p, p, p), "NULL sum")
        _rejected(lib, name, (ctx, None, None, 4, 1, p, p, p), "NULL sum")
        _rejected(lib, name, (ctx, p, None, 4, 1, p, p, p), "NULL count")
    _rejected(lib, name, (None, p, p, 4, 1, p, p, p), "NULL context")
    _rejected(lib, name, (None, None, None, 0, 1, p, p, p), "NULL context")
    for args in ((fake, None, None, 0, 1, p, p, p), (fake, p, p, 0, capi.TONEMAP_ALL, None, None, p),
                 (fake, None, p, 0, capi.TONEMAP_NONE, None, p, None)):
        assert getattr(lib, name)(*args) == capi.RT_OK, args


def test_debug_entry_rejects_null(lib):
    n = ctypes.c_uint32(7)
    assert lib.rt_debug_adaptive_listed(None, ctypes.byref(n)) == capi.RT_ERR_INVALID_ARG
    assert lib.rt_last_error().endswith(b"rt_debug_adaptive_listed")
    buf = np.zeros(8, np.float64)
    assert lib.rt_debug_adaptive_listed(buf.ctypes.data, None) == capi.RT_ERR_INVALID_ARG


def test_binding_lists_the_entries():
    assert set(ADAPTIVE + RESOLVE + ("rt_debug_adaptive_listed",)) <= set(capi.EXPORTED)
    for m in ("accumulate_adaptive", "accumulate_adaptive_device", "resolve_counts",
              "resolve_counts_device", "render_adaptive"):
        assert hasattr(capi.DeviceScene, m), m
    assert hasattr(capi.Context, "debug_adaptive_listed")
    assert capi.AdaptiveState._fields == ("sum", "moments", "count")
    assert ctypes.sizeof(capi.AdaptiveRule) == 24
    with open(os.path.join(ROOT, "include", "rt_capi.h")) as fh:
        header = fh.read()
    for name in ADAPTIVE + RESOLVE + ("rt_debug_adaptive_listed",):
        assert re.search(rf"\nrt_status {name}\(", header), name
    doc = header.split("rt_status rt_accumulate_adaptive_device(")[0][-6000:]
    for text in ("Scene.h:289-297", "err2 = var / nd", "return err2 <= lim*lim",
                 "typedef struct rt_adaptive_rule", "RTAMD_ADAPT_LIST=0"):
        assert text in doc, text
    assert "Scene.h:298-303" in header.split("rt_status rt_resolve_counts_device(")[0][-1500:]


def test_kernel_source_is_in_the_recipe_and_the_digest():
    assert "rt_adaptive.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "rt_adaptive.hip"))
    assert len(build.source_digest()) == 64
    with open(os.path.join(build.CSRC, "rt_internal.hpp")) as fh:
        internal = fh.read()
    assert "launch_accumulate_adaptive(" in internal and "launch_resolve_counts(" in internal
    with open(os.path.join(build.CSRC, "rt_adaptive.hip")) as fh:
        src = fh.read()
    assert "#pragma clang fp contract(off)" in src
    # the rule and the loop body are written once: one definition, called by both kernels
    for fn in ("adaptive_converged", "adaptive_sample"):
        assert len(re.findall(rf"__device__ __forceinline__ \w+ {fn}\(", src)) == 1, fn
    assert src.count("adaptive_sample<PATH>(") == 2


def test_register_and_private_memory_budget():
    """adaptive_tile_kernel<PATH> and adaptive_list_kernel<PATH>, one per TraceRay shape: at least
    2 waves per SIMD (at most 256 VGPRs + AGPRs) and no more private memory per lane than
    accumulate_samples_kernel<PATH> of the same build.  resolve_counts_kernel has no private
    segment."""
    ad = _kernels("rt_adaptive.hip")
    acc = {n: r for n, r in _kernels("rt_accumulate.hip").items() if "accumulate_samples_kernel" in n}
    res = [r for n, r in ad.items() if "resolve_counts_kernel" in n]
    assert len(ad) == 7 and len(acc) == 3 and len(res) == 1, (sorted(ad), sorted(acc))
    for path in (0, 1, 2):
        _, apriv = next(r for n, r in acc.items() if f"accumulate_samples_kernelILi{path}EE" in n)
        for kind in ("tile", "list"):
            name, (regs, priv) = next((n, r) for n, r in ad.items()
                                      if f"adaptive_{kind}_kernelILi{path}EE" in n)
            print(f"path {path}: adaptive_{kind}_kernel {regs} registers, {priv} B private; "
                  f"accumulate_samples_kernel {apriv} B private")
            alloc = max(8, -(-regs // 8) * 8)
            assert min(8, 512 // alloc) >= 2, (name, regs)
            assert priv <= apriv, (name, priv, apriv)
    print(f"resolve_counts_kernel: {res[0][0]} registers, {res[0][1]} B private")
    assert res[0][1] == 0


def test_cpp_example_compiles():
    """examples/adaptive_scenefile.cpp is registered in the build recipe and links against the
    drop-in API, with Scene::AccumulateAdaptive and the count overloads of rtamd::resolve resolved
    by librtamd_cpp.so; with wrong arguments it prints its usage and exits 2."""
    assert build.EXAMPLES.get("adaptive_scenefile") == "adaptive_scenefile.cpp"
    build.build_cpp_api()
    exe = os.path.join(ROOT, "examples", "bin", "adaptive_scenefile")
    assert os.path.exists(exe)
    syms = subprocess.run(["nm", "-C", "-u", exe], capture_output=True, text=True, check=True).stdout
    assert "Scene::AccumulateAdaptive(int, rtamd::AdaptiveRule const&, rtamd::AdaptiveState&) const" in syms
    assert re.search(r"rtamd::resolve\(std::vector<Vec3.*std::vector<int", syms)
    assert re.search(r"rtamd::resolveTonemapped\(std::vector<Vec3.*std::vector<int.*, int\)", syms)
    for args in ([], ["--check"], ["--check", "a"], ["a", "b", "c", "d"], ["a", "b", "-1"],
                 ["a", "b", "nan"], ["a", "b", "0.1x"]):
        run = subprocess.run([exe, *args], capture_output=True, text=True)
        assert run.returncode == 2 and "usage" in run.stderr, args


# ------------------------------------------------------------------ the rule on the oracle's samples
@pytest.fixture(scope="module")
def oracle_samples(oracle):
    """Per scene of adaptive_sets.FRAMES, made once: TraceRay of the C oracle for the camera ray
    of every sample of every pixel, [AA][n,3]."""
    cache = {}

    def get(name):
        if name not in cache:
            w, h = FRAMES[name]
            sc = make_config(name, w, h, aa=AA)
            per = []
            for s in range(AA):
                rays = np.array([oracle.get_ray(sc, x, y, s > 0, SEED, s)
                                 for y in range(h) for x in range(w)])
                per.append(oracle.trace_rays(sc, rays)[0])
            cache[name] = per
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_inputs_are_adversarial(oracle_samples, name):
    """On every frame the GPU tests use, the rule stops pixels at every count from min_samples = 2
    to aa = 8: each exit of the loop, and each length of a continued range, is exercised."""
    count, total, moments = stop_counts(oracle_samples(name), RULE, AA)
    hist = np.bincount(count, minlength=AA + 1)
    print(f"{name}: counts 2..8 {hist[2:].tolist()}")
    assert hist[:2].sum() == 0 and (hist[2:] > 0).all(), hist
    assert np.isfinite(total).all() and np.isfinite(moments).all()
    # never converging: the plain fold
    n8, t8, _ = stop_counts(oracle_samples(name), dict(RULE, min_samples=AA), AA)
    acc = np.zeros_like(t8)
    for s in range(AA):
        acc = acc + oracle_samples(name)[s]
    assert (n8 == AA).all() and t8.tobytes() == acc.tobytes()


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_stop_counts_is_cut_invariant(oracle_samples, name):
    per = oracle_samples(name)
    whole = stop_counts(per, RULE, AA)
    state = None
    for end in (3, 5, 8):
        before = state
        state = stop_counts(per, RULE, end, start=state)
        one = stop_counts(per, RULE, end)
        for a, b in zip(state, one):
            assert a.tobytes() == b.tobytes(), (name, end)
        if before is not None:  # a pixel the rule stopped stays stopped
            stopped = before[0] < {5: 3, 8: 5}[end]
            assert stopped.any()
            for a, b in zip(state, before):
                assert a[stopped].tobytes() == b[stopped].tobytes(), (name, end)
    for a, b in zip(state, whole):
        assert a.tobytes() == b.tobytes(), name


def test_converged_handles_nan_and_zero():
    n = np.array([2, 2, 3, 4], np.int32)
    m1 = np.array([np.nan, 0.0, 3.0, np.inf])
    m2 = np.array([1.0, 0.0, 3.0, np.inf])
    got = adaptive_sets.converged(n, m1, m2, 0.05, 0.01)
    assert got.tolist() == [False, True, True, False]
