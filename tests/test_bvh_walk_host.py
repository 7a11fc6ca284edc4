"""The three triangle-BVH traversals restated on the host against the ordered loop over all
triangles: tests/bvh_walk/walk_main.cpp, a stand-alone program with its own main, built here with
g++ against the real builder (csrc/rt_bvh.cpp) and the C oracle.  It restates bvh_box_v, the
per-lane walk (bvh_triangles, csrc/rt_trace_common.hpp), the any-hit walk (any_bvh_triangles,
csrc/rt_anyhit_device.hpp) and the wave-coherent walk of the packet kernels (bvh_wave,
csrc/rt_packet_device.hpp) over 64 emulated lanes, and runs them on random meshes and on the
crafted scenes of tests/mesh_sets.py: every walk returns exactly the loop's (t, index), more than
a million rays per run.  Its depth mode holds the claim behind kBvhStack = kPkStack = 64 (a
comment, "depth <= 48", until now): on the fan mesh the builder reaches its depth cap, 48, and no
walk's stack pointer passes depth + 1.  The scenes of mesh_sets.DEPTH_CAP go to a GPU only with
this passing.  CPU only.
"""
import os
import re
import subprocess

import pytest

import mesh_sets as ms
from host_programs import ROOT, build

SRC = "tests/bvh_walk/walk_main.cpp"
BVH = dict(sources=["raytracingengine_amd/csrc/rt_bvh.cpp"],
           cxx_extra=["-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"])
SEED, CASES = 20261021, 2000     # about 10 s on 8 cores
CRAFTED = [n for n in ms.SCENES if n not in ("fan_spheres", "wall_nolight")]  # (meshes seen already)


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    d = tmp_path_factory.mktemp("walk")
    exe = build(d, "walk_main", SRC, [], **BVH)
    files = {}
    for name in CRAFTED:
        files[name] = str(d / f"{name}.txt")
        with open(files[name], "w") as fh:
            fh.write(ms.hex_scene(ms.SCENES[name]()))
    return exe, files


def _run(exe, *args, env=None, timeout=300):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=timeout,
                       env=env)
    print(r.stdout, r.stderr[-2000:])
    return r, {k: int(v) for k, v in re.findall(r"(\w+) (-?\d+)", r.stdout.splitlines()[-1])} \
        if r.stdout else {}


def _pk_stack():
    with open(os.path.join(ROOT, "raytracingengine_amd", "csrc", "rt_packet_device.hpp")) as fh:
        return int(re.search(r"constexpr int kPkStack = (\d+);", fh.read()).group(1))


def test_every_walk_returns_the_loops_hit(walk):
    exe, files = walk
    r, f = _run(exe, "prop", SEED, CASES, *files.values())
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert f["bad_wave"] == 0 and f["bad_lane"] == 0 and f["bad_any"] == 0
    assert f["rays"] >= 10 ** 6
    assert 4 * f["hits"] >= f["rays"]          # the rays are aimed: at least one in four hits
    assert f["max_sp"] == 49                   # the fan's spine was walked


def test_depth_cap_and_stack_use(walk):
    """The fan: the tree's depth is the builder's cap, the d.x == 0 column reaches the leaf at the
    cap, and every walk's largest stack pointer is depth + 1 = 49, below both stacks' 64."""
    exe, files = walk
    pk = _pk_stack()
    r, f = _run(exe, "depth", pk, files["fan"])
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    first = {k: int(v) for k, v in re.findall(r"(\w+) (-?\d+)", r.stdout.splitlines()[0])}
    assert first["depth"] == 48 and first["column_leaf"] == 48
    assert first["max_sp"] <= first["depth"] + 1 < min(first["kBvhStack"], pk)
    assert first["kPkStack"] == pk == 64 and first["kBvhStack"] == 64
    assert f["bad_wave"] == 0 and f["bad_lane"] == 0 and f["bad_any"] == 0


@pytest.mark.parametrize("mutation,where", [("notie", "bad_wave"), ("nomargin", "bad_wave"),
                                            ("nowiden", "bad_lane")])
def test_mutations_are_caught(walk, mutation, where):
    """The program is not vacuous: the wave walk without its 'i < ti' tie rule, the wave walk
    pruning at tn > bound without the 1e-9 margin, and node boxes without the builder's widening
    each make it fail."""
    exe, files = walk
    r, f = _run(exe, "prop", SEED, 100, "--mutate", mutation, files["wall"], files["floor"])
    assert r.returncode == 1, (mutation, r.returncode, r.stdout[-2000:])
    assert f[where] > 0, (mutation, f)


def test_host_program_under_sanitizers(tmp_path, walk):
    """The same stand-alone program, and the builder in it, with AddressSanitizer and UBSan."""
    _, files = walk
    exe = build(tmp_path, "walk_main_san", SRC,
                ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                 "-fno-omit-frame-pointer"], **BVH)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for args in (("prop", SEED, 10, files["wall_60x44"], files["fan_f48"], files["inside"]),
                 ("depth", _pk_stack(), files["fan"])):
        r, f = _run(exe, *args, env=env)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
        assert f["bad_wave"] == 0 and f["bad_lane"] == 0 and f["bad_any"] == 0
