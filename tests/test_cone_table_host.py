"""The camera-cone mask table's host-callable math (csrc/rt_cone_table.hpp) against the C oracle:
tests/cone_table/cone_main.cpp, a stand-alone program with its own main, built here with g++ and
run on random cameras (off-axis ones included), focal lengths 0.05..100, frame sizes that are no
multiple of 8, the row plans (begin 1, block 2, cycle 2), (block 3, cycle 3), (block 8, cycle 2)
and spheres from sub-pixel to screen-filling, behind, around and next to the camera and with
|oc|/r > 1e5.  Property: for every tile and every pixel of it, a sphere whose FP64 intersection
with the pixel's ray (oracle_sphere_intersect) yields a root >= 1e-6 has its bit set in the
tile's mask.  CPU only.
"""
import re
import subprocess

import pytest

from host_programs import build
from raytracingengine_amd.configs import make_config

SEED, CASES = 20240607, 400


@pytest.fixture(scope="module")
def cone_main(tmp_path_factory):
    d = tmp_path_factory.mktemp("cone")
    exe = build(d, "cone_main", "tests/cone_table/cone_main.cpp", [])
    return exe, d


def _fields(line):
    return {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", line)}


def test_every_hit_sphere_is_in_its_tiles_mask(cone_main):
    exe, _ = cone_main
    r = subprocess.run([exe, "prop", str(SEED), str(CASES)], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    f = _fields(r.stdout)
    assert f["missed"] == 0
    assert f["hits"] >= 10000
    # the sample culls: at least one tile in ten keeps some spheres and drops others
    assert 10 * f["partial"] >= f["tiles"]


def test_c2_frame_popcounts(cone_main):
    """The C2 frame at 1920x1080: the table's candidates in total do not exceed those of the
    per-wave cull it replaces (same pixel extents, centred axis; measured 2 691 against 2 736,
    the other axis keeping a sphere more in 4 of the 32 400 tiles)."""
    exe, d = cone_main
    sc = make_config("c2")
    cam = sc.camera
    path = d / "c2.txt"
    with open(path, "w") as fh:
        fh.write(f"{cam.width} {cam.height} " +
                 " ".join(float(v).hex() for v in (*cam.position, cam.focal)) + "\n")
        for s in sc.spheres:
            fh.write(" ".join(float(v).hex() for v in (*s[0], s[1])) + "\n")
    r = subprocess.run([exe, "frame", str(path)], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    f = _fields(r.stdout)
    assert f["tiles"] == 240 * 135
    assert 0 < f["table_popcount"] <= f["wave_popcount"]
