"""The tile class words' host-callable rule (tile_class_word, csrc/rt_shadow_table.hpp) against
the C oracle: tests/tile_class/class_main.cpp, a stand-alone program with its own main, built here
with g++ like tests/test_shadow_table_host.py's and run on the same random frames (off-axis
cameras, focal lengths 0.05..100, frame sizes that are no multiple of 8, the three row plans, 1..5
planes with twins and tilts, 1..4 lights).

Properties.  Every lane pixel (clamped as the kernel clamps) of every tile that meets the class's
geometric conditions — empty cone mask, at most one kept plane, which leads by the class margin
and has a valid oriented normal: `single` — has the class's plane as oracle_closest's hit, or a
miss for a sky tile; and no shadow ray the oracle casts from a uniform tile (a `single` tile whose
shadow words are all zero: the tiles that get a class word) has a sphere root in [1e-6, maxDist].

Measured with the class margin of 1e-6 over the 2 000 cases: 21 338 single tiles (21 500 under
the shadow words' 1e-9 rule alone), 1 631 of them sky, 6 683 tiles whose shadow words are all
zero, 6 488 uniform tiles, 0 violations; the floors below are about 70 % of these.  The floor of
15 000 is on the single tiles: the uniform ones are a subset of the zero-word tiles, and the
closest-hit property is checked on every single tile, which is the larger set.  Three mutants
must report violations.  CPU only.
"""
import os
import re
import subprocess

import pytest

from host_programs import build, write_frame_file
from raytracingengine_amd.configs import make_config

SEED, CASES = 20240607, 2000
SRC = "tests/tile_class/class_main.cpp"


@pytest.fixture(scope="module")
def class_main(tmp_path_factory):
    d = tmp_path_factory.mktemp("tile_class")
    return build(d, "class_main", SRC, []), d


def _fields(line):
    return {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", line)}


def _prop(exe, cases, mutant="none", env=None):
    r = subprocess.run([exe, "prop", str(SEED), str(cases), mutant], capture_output=True,
                       text=True, timeout=300, env=env)
    print(r.stdout, r.stderr[-2000:])
    return r, _fields(r.stdout)


def test_uniform_tiles_see_their_plane_and_cast_no_shadowed_ray(class_main):
    exe, _ = class_main
    r, f = _prop(exe, CASES)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    assert f["violations"] == 0
    assert f["single"] >= 15000
    assert f["sky"] >= 1000
    assert f["zero_words"] >= 4000
    assert f["uniform"] >= 4500


@pytest.mark.parametrize("mutant", ["two", "hide", "index"])
def test_mutants_report_violations(class_main, mutant):
    """The class taken on two kept planes, hidden and leading decided on one corner, the kept
    plane's index off by one: each names a plane some pixel of the tile does not see."""
    exe, _ = class_main
    r, f = _prop(exe, CASES, mutant)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    assert f["single"] >= 15000
    assert f["violations"] > 0


def test_c2_frame(class_main):
    """The C2 frame at 1920x1080: at least 70 % of the 32 400 tiles are uniform and at least 65 %
    of the 16 200 workgroups have both waves uniform (measured: 23 458 tiles, 11 608
    workgroups), with no violation."""
    exe, d = class_main
    sc = make_config("c2")
    path = d / "c2.txt"
    write_frame_file(path, sc, 1e-3)
    r = subprocess.run([exe, "frame", str(path)], capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    f = _fields(r.stdout)
    assert f["tiles"] == 240 * 135 and f["workgroups"] == 120 * 135
    assert f["violations"] == 0
    assert 100 * f["uniform"] >= 70 * f["tiles"]
    assert 100 * f["uniform_wgs"] >= 65 * f["workgroups"]


def test_host_program_under_sanitizers(tmp_path):
    """The same stand-alone program with AddressSanitizer and UBSan, on a short case count."""
    exe = build(tmp_path, "class_main_san", SRC,
                ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                 "-fno-omit-frame-pointer"])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for mutant in ("none", "two", "hide", "index"):
        r, f = _prop(exe, 60, mutant, env)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
        if mutant == "none":
            assert f["violations"] == 0
