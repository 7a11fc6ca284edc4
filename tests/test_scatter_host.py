"""The scatter query (rt_scatter_rays / rt_scatter_rays_device) as far as it goes without a
device: argument checks, the bindings, the build recipe, the C++ example, and the register and
private-memory budget of the built gfx950 kernels next to the kernels they share code with."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from raytracingengine_amd import build, capi
from test_anyhit_host import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rt_scatter_rays", "rt_scatter_rays_device")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return capi.load_library()


def _call(lib, name, inputs=True, outputs=capi.SC_ALL, out="all", n=4):
    """One call with a NULL context and scene: nothing can reach a device."""
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data
    ptrs = capi.ScatterPtrs(p, p, p, p, p) if out == "all" else out
    ref = ctypes.byref(ptrs) if ptrs is not None else None
    st = getattr(lib, name)(None, None, None, p if inputs else None, n, outputs, ref)
    return st, lib.rt_last_error()


@pytest.mark.parametrize("name", ENTRIES)
def test_bad_arguments_rejected(lib, name):
    """RT_ERR_INVALID_ARG before anything touches a device, each with its own message ending in
    the entry's name: no output bit, an unknown bit, a NULL record, a requested output whose
    pointer is NULL, NULL rays with n > 0, and a NULL context."""
    p = np.zeros(8, np.float64).ctypes.data
    cases = {
        "no output": dict(outputs=0),
        "unknown output bit": dict(outputs=0x20 | capi.SC_VALUE),
        "NULL output record": dict(out=None),
        "NULL pointer of a requested output": dict(outputs=capi.SC_WEIGHTS,
                                                   out=capi.ScatterPtrs(p, p, p, None, p)),
        "NULL argument": dict(inputs=False),
        "NULL context": dict(),
    }
    for text, kw in cases.items():
        st, msg = _call(lib, name, **kw)
        assert st == capi.RT_ERR_INVALID_ARG, (name, text)
        assert text.encode() in msg and msg.endswith(name.encode()), (text, msg)
    for bit, field in zip((1, 2, 4, 8, 16), [f for f, _ in capi.ScatterPtrs._fields_]):
        ptrs = capi.ScatterPtrs(p, p, p, p, p)
        setattr(ptrs, field, None)
        st, msg = _call(lib, name, outputs=bit, out=ptrs)
        assert st == capi.RT_ERR_INVALID_ARG and b"NULL pointer of a requested output" in msg, field
        # pointers of outputs that were not requested are not looked at: the call gets as far as
        # the context check
        st, msg = _call(lib, name, outputs=capi.SC_ALL & ~bit, out=ptrs)
        assert st == capi.RT_ERR_INVALID_ARG and b"NULL context" in msg, field
    # n == 0 with NULL rays passes the argument checks and stops at the context
    st, msg = _call(lib, name, inputs=False, n=0)
    assert st == capi.RT_ERR_INVALID_ARG and b"NULL context" in msg


def test_binding_lists_the_entries():
    assert set(ENTRIES) <= set(capi.EXPORTED)
    for m in ("scatter", "scatter_device"):
        assert hasattr(capi.DeviceScene, m), m
    assert callable(capi.compose_trace)
    assert (capi.SC_VALUE, capi.SC_REFRACT, capi.SC_REFLECT, capi.SC_WEIGHTS, capi.SC_FLAGS,
            capi.SC_ALL) == (1, 2, 4, 8, 16, 31)
    assert [n for n, _ in capi.ScatterPtrs._fields_] == ["value", "refract_rays", "reflect_rays",
                                                         "weights", "flags"]
    with open(os.path.join(ROOT, "include", "rt_capi.h")) as fh:
        header = fh.read()
    for name, value in (("RT_SC_VALUE", 1), ("RT_SC_REFRACT", 2), ("RT_SC_REFLECT", 4),
                        ("RT_SC_WEIGHTS", 8), ("RT_SC_FLAGS", 16), ("RT_SC_ALL", 31)):
        line = next(l for l in header.splitlines() if l.startswith(f"#define {name} "))
        assert int(line.split()[2], 16) == value, line


def test_kernel_source_is_in_the_digest():
    assert "rt_scatter.hip" in build.SOURCES
    # the digest covers SOURCES and every csrc file by name and bytes
    assert os.path.exists(os.path.join(build.CSRC, "rt_scatter.hip"))
    assert len(build.source_digest()) == 64


def test_cpp_example_compiles():
    """examples/scatter_scenefile.cpp is registered in the build recipe and links against the
    drop-in API, with Scene::ScatterRays resolved by librtamd_cpp.so; without arguments it prints
    its usage."""
    assert build.EXAMPLES.get("scatter_scenefile") == "scatter_scenefile.cpp"
    build.build_cpp_api()
    exe = os.path.join(ROOT, "examples", "bin", "scatter_scenefile")
    assert os.path.exists(exe)
    syms = subprocess.run(["nm", "-C", "-u", exe], capture_output=True, text=True, check=True).stdout
    assert "Scene::ScatterRays(std::vector<Rayon" in syms
    assert "Scene::TraceRays(std::vector<Rayon" in syms
    for args in ([], ["--depth", "2"], ["--depth", "2", "a", "b"]):
        run = subprocess.run([exe, *args], capture_output=True, text=True)
        assert run.returncode == 2 and "usage" in run.stderr


def test_register_budget():
    """The BVH stack is the kernels' only private memory — their private segments are no larger
    than direct_light_rays_kernel's, so nothing spills — and they hold no more registers than
    trace_rays_kernel<kPathTree, false>, which runs the same level plus the recursion.  Three
    instances per TREE: value and children, value alone, children alone."""
    sk = {n: r for n, r in _kernels("rt_scatter.hip").items() if "scatter_rays_kernel" in n}
    assert len(sk) == 6, sorted(sk)
    rays = [r for n, r in _kernels("rt_direct.hip").items() if "direct_light_rays_kernel" in n]
    # trace_rays_kernel<PATH = kPathTree = 2, COUNT = false>: _ZN5rtamd17trace_rays_kernelILi2ELb0EEE...
    tree = [r for n, r in _kernels("rt_trace.hip").items() if "trace_rays_kernelILi2ELb0EE" in n]
    assert len(rays) == 2 and len(tree) == 1
    rpriv = min(priv for _, priv in rays)
    tregs = tree[0][0]
    print(f"direct_light_rays_kernel {rpriv} B private; trace_rays_kernel<tree> {tregs} registers")
    for name, (regs, priv) in sorted(sk.items()):
        print(f"{name}: {regs} registers, {priv} B private")
        assert priv <= rpriv, name
        assert regs <= tregs, name
