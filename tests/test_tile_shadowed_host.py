"""The shadowed-plane tiles' host-callable rule and lists (tile_shadowed_mark, tile_shadowed_entry
and tile_list_run, csrc/rt_shadow_table.hpp: what one lane and one wavefront of the table kernel
do): tests/tile_shadowed/shadowed_main.cpp, a stand-alone program with its own main, built here
with g++ like tests/test_tile_lists_host.py's and run on the same 2 000 random frames and on the
C2 frame.

Properties, per frame: every lane pixel of a shadowed tile has the oracle's closest hit on the
plane its list entry names; every sphere a shadow ray of such a pixel meets with a root in
[1e-6, maxDist] is in that light's word; every 8x8 tile is in exactly one of the uniform list, the
shadowed list and the general waves of a listed workgroup; a workgroup is listed if and only if it
has a tile that is neither uniform nor shadowed; each entry decodes to its tile, its plane and its
keep masks.  Three mutants must be caught: the shadowed class taken when a light has no word, an
entry's plane index off by one, and a workgroup with a shadowed wave and a general wave dropped
from the general list.  CPU only.
"""
import re
import subprocess

import pytest

from host_programs import build, write_frame_file
from raytracingengine_amd.configs import make_config

SEED, CASES = 20240607, 2000
SRC = "tests/tile_shadowed/shadowed_main.cpp"


@pytest.fixture(scope="module")
def shadowed_main(tmp_path_factory):
    d = tmp_path_factory.mktemp("tile_shadowed")
    return build(d, "shadowed_main", SRC, []), d


def _fields(line):
    return {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", line)}


def _prop(exe, cases, mutant="none"):
    r = subprocess.run([exe, "prop", str(SEED), str(cases), mutant], capture_output=True,
                       text=True, timeout=300)
    print(r.stdout, r.stderr[-2000:])
    return r, _fields(r.stdout)


def test_shadowed_tiles_hold_and_every_tile_is_listed_once(shadowed_main):
    """(measured: 14 850 shadowed tiles, 2 590 workgroups with a shadowed and
    a general wave; the floors are about 70 % of the measured figures)"""
    exe, _ = shadowed_main
    r, f = _prop(exe, CASES)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    assert f["violations"] == 0
    assert f["shadowed"] >= 10400
    assert f["mixed"] >= 1800
    assert f["rays"] > 0 and f["pixels"] == 64 * f["shadowed"]
    assert f["cand1"] + f["cand2"] + f["cand3"] == f["shadowed"]
    assert 0 < f["listed"] < f["general_wgs"] < f["workgroups"]


@pytest.mark.parametrize("mutant", ["noword", "index", "mixed"])
def test_mutants_report_violations(shadowed_main, mutant):
    exe, _ = shadowed_main
    r, f = _prop(exe, CASES, mutant)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    assert f["shadowed"] >= 10400
    assert f["violations"] > 0


def _c2_file(d):
    sc = make_config("c2")
    path = d / "c2.txt"
    write_frame_file(path, sc, 1e-3)
    return path


def test_c2_frame(shadowed_main):
    """The C2 frame at 1920x1080: 23 458 uniform tiles, 6 032 shadowed tiles and 1 550 listed
    workgroups (4 592 without the shadowed list), no violation; the census mode prints the same
    counts (profiles/tile_shadowed_census.txt)."""
    exe, d = shadowed_main
    path = _c2_file(d)
    r = subprocess.run([exe, "frame", str(path)], capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    f = _fields(r.stdout)
    assert f["tiles"] == 240 * 135 and f["workgroups"] == 120 * 135
    assert f["violations"] == 0
    assert f["uniform"] == 23458
    assert f["shadowed"] == 6032
    assert f["listed"] == 1550
    assert f["general_wgs"] == 4592
    assert (f["cand1"], f["cand2"], f["cand3"]) == (5144, 750, 138)
    c = subprocess.run([exe, "census", str(path)], capture_output=True, text=True, timeout=600)
    print(c.stdout, c.stderr[-2000:])
    assert c.returncode == 0
    assert re.search(r"shadowed .* 6032\n", c.stdout) and re.search(r"listed\) +1550\n", c.stdout)
