"""The staging layout of the host batch queries (csrc/rt_stage.hpp: where the inputs and outputs
of one query sit in the context's staging buffer): tests/stage/stage_main.cpp, a stand-alone
program with its own main that includes that header only, built here with g++ like
tests/test_tile_lists_host.py's, and a second time with -fsanitize=address,undefined and run
directly.

It declares the items of every host entry for n in {0, 1, 63, 64, 65, 257}, every output mask of
the three output records and 0, 1 and 3 lights.  Properties, per case: the total is the bytes the
entry has always asked for; no two items overlap; an item whose size is a multiple of 8 is 8-byte
aligned; an output that was not requested has no extent; offsets follow the declaration order,
the byte-sized items last.  Two mutants must be caught: an item's offset short by its
predecessor's last byte, and the byte-sized output placed before a double output (n odd).
CPU only.
"""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "stage" / "stage_main.cpp"
# per n: trace, intersect, occluded, transmittance, 3 light counts, camera; 3 x 7 direct-light
# masks; 31 scatter and 31 closest masks
CASES = 6 * (4 + 3 + 1 + 3 * 7 + 2 * 31)


def _build(d, name, extra):
    exe = str(d / name)
    subprocess.run(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-Werror", *extra,
                    f"-I{ROOT}/raytracingengine_amd/csrc", str(SRC), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("stage")


@pytest.fixture(scope="module")
def stage_main(build_dir):
    return _build(build_dir, "stage_main", [])


def _run(exe, mutant="none"):
    r = subprocess.run([exe, mutant], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    return r, {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", r.stdout)}


def test_the_header_has_no_hip_include():
    text = (ROOT / "raytracingengine_amd" / "csrc" / "rt_stage.hpp").read_text()
    assert re.findall(r"#include\s+[<\"]([^>\"]+)", text) == ["cstddef"]


def test_every_entry_layout(stage_main):
    r, f = _run(stage_main)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    assert f["cases"] == CASES
    assert f["violations"] == 0
    assert (f["total"], f["overlap"], f["aligned"], f["extent"], f["order"]) == (0, 0, 0, 0, 0)


def test_every_entry_layout_under_sanitizers(build_dir):
    exe = _build(build_dir, "stage_main_san",
                 ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r, f = _run(exe)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    assert f["cases"] == CASES and f["violations"] == 0
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


@pytest.mark.parametrize("mutant,caught_by", [("short", "overlap"), ("bytes", "aligned")])
def test_mutants_report_violations(stage_main, mutant, caught_by):
    """short: every case with two items that have bytes overlaps (n > 0); bytes: the cases with a
    byte-sized output and odd n leave a double item off its alignment."""
    r, f = _run(stage_main, mutant)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    assert f["cases"] == CASES
    assert f[caught_by] > 0 and f["violations"] > 0
