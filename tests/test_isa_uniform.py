"""Per-lane VALU work on wave-uniform values stays out of the packet kernels (no GPU).

FP64 has no scalar ALU on gfx950: an expression of kernel arguments alone (W/2, H/2, the camera
ray's dz and dz·dz) compiles to VALU instructions that every lane of every wave executes for one
value per frame.  The host forms such values once per frame (camera_consts, rt_internal.hpp).
tools/isa/census.py --uniform lists what is left: VALU arithmetic and conversion instructions
whose sources are all SGPRs, literals or inline constants (through v_mov inside a block).  This
test compiles the four packet variants the BASELINE configs run and holds the listing to the
counts of the commit before the frame constants moved to the host.
"""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# <MAXC, FEAT, COUNT, MULTI, WGY> of packet_direct_kernel
VARIANTS = {"c2_fixup": "1,128,false,false,1", "c2_march": "1,0,false,false,1",
            "c3_c4": "4,0,false,false,1", "c5_area": "1,34,false,false,1"}
# census.py --uniform of the parent commit (a947131), same compiler and flags as below
PARENT_UNIFORM = {"c2_fixup": 43, "c2_march": 56, "c3_c4": 53, "c5_area": 107}


def _census():
    spec = importlib.util.spec_from_file_location(
        "isa_census", os.path.join(ROOT, "tools", "isa", "census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    """{variant: blocks of its packet_direct_kernel}; the four probes compile side by side."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("isa_uniform")
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


@pytest.mark.parametrize("name", ["c2_fixup", "c2_march"])
def test_no_int_to_double_conversion_of_a_scalar(listings, name):
    """Camera::getRay's W/2 and H/2 come from the kernel arguments: the only v_cvt_f64_u32 left
    are the per-lane ones of the pixel's x and y, which take a VGPR."""
    _, res = listings
    cvts = [l for ins in res[name].values() for l in ins if l.startswith("v_cvt_f64_u32")]
    assert len(cvts) >= 2, "the camera ray's per-lane conversions of x and y are gone"
    scalar = [l for l in cvts if re.search(r",\s*s\d+\s*$", l) or re.search(r",\s*s\[", l)]
    assert scalar == []


@pytest.mark.parametrize("name", list(VARIANTS))
def test_uniform_valu_not_above_parent(listings, name):
    census, res = listings
    hits = census.uniform_valu(res[name])
    print(f"{name}: {len(hits)} uniform-source VALU instructions (parent {PARENT_UNIFORM[name]})")
    assert len(hits) <= PARENT_UNIFORM[name], "\n".join(f"{b} {l}" for b, l in hits)


# a listing of a few lines for --uniform itself
FIXTURE = {
    ".LBB0_1": [
        "s_load_dwordx2 s[4:5], s[0:1], 0x10",
        "v_mov_b32_e32 v4, s6",                      # uniform copy
        "v_cvt_f64_u32_e32 v[2:3], v4",              # 1: through the v_mov
        "v_mul_f64 v[2:3], v[2:3], 0.5",             # 2: through the reported conversion
        "v_add_f64 v[8:9], s[4:5], v[2:3]",          # 3: SGPR pair + uniform VGPR pair
        "v_add_f64 v[10:11], v[8:9], -v[20:21]",     # mixed: v[20:21] is per-lane
        "v_mul_f64 v[12:13], v[10:11], v[10:11]",    # per-lane (its source was mixed)
        "v_cndmask_b32_e64 v5, 0, 1.0, s[8:9]",      # reads a lane mask
        "v_mbcnt_lo_u32_b32 v6, -1, 0",              # reads the lane number
        "v_mul_f32_e64 v7, |s9|, 0x3f8020c5",        # 4: modifiers and a literal
        "global_load_dwordx2 v[2:3], v[30:31], off",
        "v_mul_f64 v[14:15], v[2:3], 2.0",           # v[2:3] was loaded: per-lane now
    ],
    ".LBB0_2": [
        "v_add_f64 v[16:17], v[8:9], 1.0",           # uniformity does not cross a block
        "v_add_co_u32_e32 v18, vcc, s2, v0",         # mixed, two destinations
        "v_mov_b32_e32 v19, v0",
        "v_add_u32_e32 v19, s3, v19",                # a v_mov from a per-lane source
    ],
}


def test_census_uniform_on_a_small_listing():
    """The fixture's uniform chain (v_mov from an SGPR, a conversion of the copy, arithmetic on
    the result) is reported instruction by instruction; an instruction with one per-lane source,
    what depends on it, lane-mask and lane-number readers, a loaded register and values carried
    across a block boundary are not."""
    census = _census()
    hits = census.uniform_valu(FIXTURE)
    assert hits == [(".LBB0_1", FIXTURE[".LBB0_1"][i]) for i in (2, 3, 4, 9)]
