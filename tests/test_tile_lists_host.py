"""The tile lists' host-callable rule (tile_list_run and its helpers, csrc/rt_shadow_table.hpp: what
one wavefront of the table kernel does with its 64 class words): tests/tile_lists/lists_main.cpp, a
stand-alone program with its own main, built here with g++ like tests/test_tile_class_host.py's
and run on the same 2 000 random frames and on the C2 frame.

Properties, per frame: every 8x8 tile is in exactly one of the uniform list (an entry that decodes
to the tile and carries its class word) and the general waves of a listed workgroup; the uniform
count is the number of class words that are not general; no tile and no workgroup is listed twice;
a workgroup is listed if and only if it has a general wave.  Two mutants must be caught: an
entry's column off by one, and a mixed workgroup (one uniform and one general wave) dropped.
CPU only.
"""
import re
import subprocess

import pytest

from host_programs import build, write_frame_file
from raytracingengine_amd.configs import make_config

SEED, CASES = 20240607, 2000
SRC = "tests/tile_lists/lists_main.cpp"


@pytest.fixture(scope="module")
def lists_main(tmp_path_factory):
    d = tmp_path_factory.mktemp("tile_lists")
    return build(d, "lists_main", SRC, []), d


def _fields(line):
    return {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", line)}


def _prop(exe, cases, mutant="none", env=None):
    r = subprocess.run([exe, "prop", str(SEED), str(cases), mutant], capture_output=True,
                       text=True, timeout=300, env=env)
    print(r.stdout, r.stderr[-2000:])
    return r, _fields(r.stdout)


def test_every_tile_is_listed_exactly_once(lists_main):
    """(measured: 6 488 uniform tiles, the count of tests/test_tile_class_host.py; the floors are
    about 70 % of the measured figures)"""
    exe, _ = lists_main
    r, f = _prop(exe, CASES)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    assert f["violations"] == 0
    assert f["uniform"] >= 4500
    assert f["mixed"] >= 100
    assert 0 < f["listed"] < f["workgroups"]


@pytest.mark.parametrize("mutant", ["index", "mixed"])
def test_mutants_report_violations(lists_main, mutant):
    exe, _ = lists_main
    r, f = _prop(exe, CASES, mutant)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    assert f["uniform"] >= 4500
    assert f["violations"] > 0


def test_c2_frame(lists_main):
    """The C2 frame at 1920x1080: the uniform list holds the 23 458 uniform tiles and the general
    list the 16 200 - 11 608 workgroups that are not wholly uniform
    (tests/test_tile_class_host.py's counts)."""
    exe, d = lists_main
    sc = make_config("c2")
    path = d / "c2.txt"
    write_frame_file(path, sc, 1e-3)
    r = subprocess.run([exe, "frame", str(path)], capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    f = _fields(r.stdout)
    assert f["tiles"] == 240 * 135 and f["workgroups"] == 120 * 135
    assert f["violations"] == 0
    assert f["uniform"] == 23458
    assert f["listed"] == 16200 - 11608
