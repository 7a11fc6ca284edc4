"""The camera ray's normalize keeps its literal-division fallback behind a branch (no GPU).

unit() (rt_device.hpp) divides through the shared-reciprocal core when the operands allow it and
through three literal divisions otherwise.  The compiler once if-converted the fallback into the
core's basic block at the camera-ray site of the packet kernels: every pixel then paid for the
core and three full IEEE divisions (~42 VALU per wave).  This test compiles the four packet
variants the BASELINE configs run (C2 fix-up and marching, C3/C4, C5) to gfx950 assembly and
checks the listing with tools/isa/census.py.
"""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# <MAXC, FEAT, COUNT, MULTI, WGY> of packet_direct_kernel
VARIANTS = {"c2_fixup": "1,128,false,false,1", "c2_march": "1,0,false,false,1",
            "c3_c4": "4,0,false,false,1", "c5_area": "1,34,false,false,1"}


def _census():
    spec = importlib.util.spec_from_file_location(
        "isa_census", os.path.join(ROOT, "tools", "isa", "census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    """{variant: blocks of its packet_direct_kernel}; the four probes compile side by side."""
    out = tmp_path_factory.mktemp("isa")
    procs = {}
    for name, v in VARIANTS.items():
        cmd = [HIPCC, "-O3", "-std=c++20", "--offload-arch=gfx950", "-ffp-contract=off",
               "-mllvm", "-amdgpu-sched-strategy=max-ilp", "--cuda-device-only", "-S",
               "-o", str(out / f"{name}.s"), f"-DRT_PACKET_PROBE={v}",
               f"-I{os.path.join(ROOT, 'include')}",
               os.path.join(ROOT, "raytracingengine_amd", "csrc", "rt_packet.hip")]
        procs[name] = subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    census = _census()
    res = {}
    for name, p in procs.items():
        _, err = p.communicate()
        assert p.returncode == 0, err.decode()[-2000:]
        found = census.kernels((out / f"{name}.s").read_text().splitlines(),
                               "packet_direct_kernel")
        assert len(found) == 1, list(found)
        res[name] = next(iter(found.values()))
    return census, res


def _camera_sqrt_block(blocks):
    """Index of the block with the camera ray's sqrt_core: the first v_rsq_f64 after the pixel
    coordinates are converted to double (v_cvt_f64_u32: Camera::getRay's sx, sy), in a block
    without the range scaling (v_ldexp_f64) of the full sqrt that serves lengths outside the
    core's range (that path rightly ends in three literal divisions)."""
    seen_cvt = False
    for i, ins in enumerate(blocks.values()):
        for l in ins:
            if l.startswith("v_cvt_f64_u32"):
                seen_cvt = True
            elif seen_cvt and l.startswith("v_rsq_f64") and \
                    not any(o.startswith("v_ldexp_f64") for o in ins):
                return i
    raise AssertionError("no v_rsq_f64 after v_cvt_f64_u32: camera ray not found")


@pytest.mark.parametrize("name", list(VARIANTS))
def test_camera_ray_normalize_is_not_folded(listings, name):
    """What every lane executes after the camera ray's square root — the block with the division
    core, which is the sqrt's own block or one of the next two (the l == 1 and component gates
    may each end a block) — holds no full division, and the three literal divisions that follow
    are entered through an exec-mask branch.  (Basic blocks end at branches here: with blocks
    split at labels only, the fallback, which falls through from its guard, would count into
    the guarded block in any build.)"""
    census, res = listings
    blocks = res[name]
    keys = list(blocks)
    i = _camera_sqrt_block(blocks)
    j = next((k for k in range(i, i + 3)
              if any(l.startswith("v_rcp_f64") for l in blocks[keys[k]])), None)
    assert j is not None, "no division core after the camera ray's sqrt"
    core = blocks[keys[j]]
    assert not any(l.startswith(("v_div_fixup_f64", "v_div_scale_f64", "v_div_fmas_f64"))
                   for l in core), f"{keys[j]}: the core's block holds full divisions"
    # the fallback: the next block with divisions is only reached past s_cbranch_execz
    d = next(k for k in range(j + 1, len(keys))
             if any(l.startswith("v_div_fixup_f64") for l in blocks[keys[k]]))
    assert blocks[keys[d - 1]][-1].startswith("s_cbranch_execz"), keys[d]
    # and no block of the kernel holds a core together with full divisions by the same divisor
    assert census.folded_blocks(blocks) == []


def test_census_folded_signature():
    """The report's signature on hand-written blocks: the parent's folded block (the core's
    v_rcp_f64 of the divisor itself and three v_div_fixup_f64 naming it) is reported; three honest
    divisions, or a core next to divisions by another value, are not."""
    census = _census()
    div = lambda d, n: [f"v_div_scale_f64 v[20:21], s[2:3], {d}, {d}, {n}",
                        "v_rcp_f64_e32 v[22:23], v[20:21]",
                        f"v_div_fixup_f64 {n}, v[22:23], {d}, {n}"]
    core = ["v_rcp_f64_e32 v[8:9], v[6:7]", "v_fma_f64 v[28:29], -v[6:7], v[8:9], 1.0"]
    three = div("v[6:7]", "v[0:1]") + div("v[6:7]", "v[2:3]") + div("v[6:7]", "v[4:5]")
    other = div("v[10:11]", "v[0:1]") + div("v[10:11]", "v[2:3]") + div("v[10:11]", "v[4:5]")
    assert census.folded_blocks({"b": core + three}) == [("b", 11, 4, 3, 3)]
    assert census.folded_blocks({"b": three}) == []
    assert census.folded_blocks({"b": core + other}) == []
    # the divisor register rewritten between the core and the divisions: another value
    assert census.folded_blocks({"b": core + ["v_mov_b64_e32 v[6:7], v[30:31]"] + three}) == []
