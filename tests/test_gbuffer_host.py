"""The G-buffer pass (rt_gbuffer / rt_gbuffer_device) as far as it goes without a device:
argument checks, the binding's constants and output shapes, the register budgets of the built
gfx950 kernels, and the C++ example."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from raytracingengine_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_capi.h")
OBJ = os.path.join(ROOT, "build", "obj")
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return capi.load_library()


def test_invalid_arguments_rejected(lib):
    """outputs == 0, an unknown bit, a NULL record and a requested output with a NULL pointer are
    RT_ERR_INVALID_ARG before anything touches a device (both entry points)."""
    buf = np.zeros(16, np.float64)
    full = capi.GBufferPtrs(*([buf.ctypes.data] * 5))
    no_depth = capi.GBufferPtrs(depth=None, depth_norm=buf.ctypes.data, normal=buf.ctypes.data,
                                prim=buf.ctypes.data, albedo=buf.ctypes.data)
    cases = [(0, ctypes.byref(full)), (0x20, ctypes.byref(full)),
             (capi.GB_ALL | 0x100, ctypes.byref(full)), (capi.GB_DEPTH, None),
             (capi.GB_DEPTH, ctypes.byref(no_depth)), (capi.GB_ALL, ctypes.byref(no_depth))]
    for outputs, ptrs in cases:
        assert lib.rt_gbuffer(None, None, None, None, outputs, ptrs) == capi.RT_ERR_INVALID_ARG
        assert b"G-buffer" in lib.rt_last_error()
        assert lib.rt_gbuffer_device(None, None, None, 1, None, outputs, ptrs) == \
            capi.RT_ERR_INVALID_ARG
        assert b"G-buffer" in lib.rt_last_error()
    # valid outputs, but no context / scene / camera
    assert lib.rt_gbuffer(None, None, None, None, capi.GB_PRIM, ctypes.byref(no_depth)) == \
        capi.RT_ERR_INVALID_ARG
    assert lib.rt_gbuffer_device(None, None, None, 1, None, capi.GB_PRIM,
                                 ctypes.byref(no_depth)) == capi.RT_ERR_INVALID_ARG


def test_constants_match_header():
    src = open(HEADER).read()
    header = {m.group(1): int(m.group(2), 16)
              for m in re.finditer(r"#define RT_GB_([A-Z_]+)\s+(0x[0-9a-fA-F]+)", src)}
    assert header == {"DEPTH": capi.GB_DEPTH, "DEPTH_NORM": capi.GB_DEPTH_NORM,
                      "NORMAL": capi.GB_NORMAL, "PRIM": capi.GB_PRIM, "ALBEDO": capi.GB_ALBEDO,
                      "ALL": capi.GB_ALL}
    assert capi.GB_ALL == (capi.GB_DEPTH | capi.GB_DEPTH_NORM | capi.GB_NORMAL | capi.GB_PRIM |
                           capi.GB_ALBEDO)
    # struct rt_gbuffer's fields, in the header's order
    body = re.search(r"struct rt_gbuffer \{(.*?)\};", src, re.S).group(1)
    assert re.findall(r"void\*\s+(\w+);", body) == [f[0] for f in capi.GBufferPtrs._fields_]
    assert ctypes.sizeof(capi.GBufferPtrs) == 5 * ctypes.sizeof(ctypes.c_void_p)


def test_layout_of_a_row_range_and_of_a_batch():
    """Shapes follow rt_render_device: rows-local, [frames,] rows, W[, k]."""
    o = capi.RenderOpts(row_begin=3, row_end=18)
    rows = capi.rendered_rows(o, 21)
    assert rows == 15
    lay = capi.gbuffer_layout(capi.GB_ALL, 37, rows)
    assert lay == {"depth": ((15, 37), np.dtype(np.float64)),
                   "depth_norm": ((15, 37), np.dtype(np.float32)),
                   "normal": ((15, 37, 3), np.dtype(np.float64)),
                   "prim": ((15, 37, 2), np.dtype(np.int32)),
                   "albedo": ((15, 37, 3), np.dtype(np.float32))}
    # block-cyclic rows of rank 1 of 3 (8-row blocks) of a 64-row frame: rows 8..15, 32..39, 56..63
    o = capi.RenderOpts(row_begin=8, row_block=8, row_cycle=3)
    lay = capi.gbuffer_layout(capi.GB_DEPTH | capi.GB_PRIM, 96, capi.rendered_rows(o, 64), 3)
    assert lay == {"depth": ((3, 24, 96), np.dtype(np.float64)),
                   "prim": ((3, 24, 96, 2), np.dtype(np.int32))}
    # bytes per pixel of every output: 8 + 4 + 24 + 8 + 12 = 56
    full = capi.gbuffer_layout(capi.GB_ALL, 1, 1)
    assert sum(int(np.prod(s)) * d.itemsize for s, d in full.values()) == 56
    for bad in (0, 0x20):
        with pytest.raises(ValueError):
            capi.gbuffer_layout(bad, 4, 4)


def _kernels():
    """{kernel name: (VGPRs + AGPRs, private segment bytes)} of build/obj/rt_gbuffer.hip.o."""
    build.build_library()
    obj = os.path.join(OBJ, "rt_gbuffer.hip.o")
    tmp = os.path.join(OBJ, "_meta_rt_gbuffer.hip")
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


def _waves(regs):
    return min(8, 512 // max(8, -(-regs // 8) * 8))


def test_register_budgets():
    """gbuffer_packet_kernel<MAXC, TRIS, TW>: the MAXC == 1 no-triangle instantiations are a strict
    subset of packet_direct_kernel<1, 0, ...> (6 waves/SIMD): at most 80 VGPRs + AGPRs and no
    private segment; the triangle variants reach RT_PACKET_TRIS_WAVES (4)."""
    ks = _kernels()
    assert any("gbuffer_generic_kernel" in n for n in ks), sorted(ks)
    packet = {n: r for n, r in ks.items() if "gbuffer_packet_kernel" in n}
    # MAXC 1, 4, 16 x triangles or not x the two tile shapes of the store A/B
    assert len(packet) == 12, sorted(packet)
    small = {n: r for n, r in packet.items() if re.search(r"kernelILi1ELb0ELi(8|16)E", n)}
    assert len(small) == 2, sorted(packet)
    assert all(regs <= 80 and priv == 0 for regs, priv in small.values()), small
    tris = {n: r for n, r in packet.items() if re.search(r"kernelILi\d+ELb1E", n)}
    assert len(tris) == 6, sorted(packet)
    assert all(_waves(regs) >= 4 for regs, _ in tris.values()), tris


def test_cpp_example_compiles():
    """examples/gbuffer_scenefile.cpp is registered in the build recipe and links against the
    drop-in API, with Scene::RenderGBuffer resolved by librtamd_cpp.so."""
    assert build.EXAMPLES.get("gbuffer_scenefile") == "gbuffer_scenefile.cpp"
    build.build_cpp_api()
    exe = os.path.join(ROOT, "examples", "bin", "gbuffer_scenefile")
    assert os.path.exists(exe)
    syms = subprocess.run(["nm", "-C", "-u", exe], capture_output=True, text=True, check=True).stdout
    assert "Scene::RenderGBuffer(int) const" in syms
    assert subprocess.run([exe], capture_output=True).returncode == 2  # usage
