"""The row plan of multi-GPU frames (csrc/rt_row_plan.hpp: which rows a rank renders, in which
slots, and where a slot sits in rank 0's receive buffer): tests/row_plan/plan_main.cpp, a
stand-alone program with its own main that includes that header only, built here with g++ like
tests/test_stage_host.py's, and a second time with -fsanitize=address,undefined and run directly.

The program plans every rank of: the eight (n, block, H) of test_assemble_rows_matches_row_planner
(among them ranks whose first block starts past H: (8, 16, 100), (16, 16, 64)); n = 1; no
row_block (the default block); root weights 1, 2, 3 and 16 with n in {2, 3, 8}.  Its own
properties, per case: every image row belongs to exactly one slot; max_rows is the maximum of the
slots' rows, the same on every rank; no slot's extent in the receive layout overlaps another's or
leaves the buffer.  Here its printed plans are compared with the independent implementation,
distributed.row_ranges / weighted_slots, and the same three properties are checked again from
the printed numbers.  One mutant must be caught: rank r >= 1 placed one slot too far.
CPU only.
"""
import re
import subprocess
from pathlib import Path

import pytest

from raytracingengine_amd.distributed import DEFAULT_BLOCK, plan_rows, row_ranges, weighted_slots

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "row_plan" / "plan_main.cpp"
CASES = 8 + 4 + 3 * 4 * 2


def _build(d, name, extra):
    exe = str(d / name)
    subprocess.run(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-Werror", *extra,
                    f"-I{ROOT}/raytracingengine_amd/csrc", f"-I{ROOT}/include", str(SRC),
                    "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("row_plan")


@pytest.fixture(scope="module")
def plan_main(build_dir):
    return _build(build_dir, "plan_main", [])


def _run(exe, mutant="none"):
    r = subprocess.run([exe, mutant], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    last = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    return r, {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", last)}


def _cases(stdout):
    """[(n, block, H, weight, {rank: (rows, max_rows, block, slots, [slot, ...])})], a slot being
    (index, rows, recv offset, recv bytes, [(a, b), ...])."""
    cases = []
    for line in stdout.splitlines():
        w = line.split()
        if w[0] == "case":
            cases.append((*map(int, w[1:5]), {}))
        elif w[0] == "rank":
            rank = int(w[1])
            cases[-1][4][rank] = (int(w[3]), int(w[5]), int(w[7]), int(w[9]), [])
        elif w[0] == "slot":
            ranges = [tuple(map(int, x.split(":"))) for x in w[8:]]
            cases[-1][4][rank][4].append((int(w[1]), int(w[3]), int(w[5]), int(w[6]), ranges))
    return cases


def test_the_header_has_no_hip_include():
    text = (ROOT / "raytracingengine_amd" / "csrc" / "rt_row_plan.hpp").read_text()
    assert re.findall(r"#include\s+[<\"]([^>\"]+)", text) == ["algorithm", "cstddef", "cstdint",
                                                               "rt_capi.h"]
    capi_h = (ROOT / "include" / "rt_capi.h").read_text()
    assert not [h for h in re.findall(r"#include\s+[<\"]([^>\"]+)", capi_h) if "hip" in h]


def test_plans_match_the_row_planner(plan_main):
    r, f = _run(plan_main)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert f == {"cases": CASES, "violations": 0, "cover": 0, "maxrows": 0, "overlap": 0}
    cases = _cases(r.stdout)
    assert len(cases) == CASES
    for n, block, H, weight, ranks in cases:
        what = (n, block, H, weight)
        assert sorted(ranks) == list(range(n)), what
        weight = 1 if n == 1 else weight  # one rank renders the whole frame
        V = weight + n - 1
        sets = [[(a, b) for a, b in row_ranges(s, V, H, block or DEFAULT_BLOCK) if a < H]
                for s in range(V)]
        max_rows = max(plan_rows(p) for p in sets)
        owners = [0] * H
        extents = []
        for rank, (rows, rank_max, rank_block, slots, mine) in ranks.items():
            assert [s[0] for s in mine] == weighted_slots(rank, n, weight), (what, rank)
            assert (rank_max, slots) == (max_rows, V), (what, rank)
            assert rank_block == (H if n == 1 else block or DEFAULT_BLOCK), (what, rank)
            assert rows == sum(s[1] for s in mine), (what, rank)
            for s, slot_rows, at, nbytes, ranges in mine:
                assert ranges == sets[s] and slot_rows == plan_rows(sets[s]), (what, rank, s)
                assert nbytes == 3 * max_rows * 7 * 24, (what, rank, s)  # frames x rows x W x bpp
                for a, b in ranges:
                    for y in range(a, b):
                        owners[y] += 1
                extents.append((at, at + nbytes))
        assert owners == [1] * H, what
        assert max(s[1] for v in ranks.values() for s in v[4]) == max_rows, what
        extents.sort()
        assert all(a[1] <= b[0] for a, b in zip(extents, extents[1:])), what
        assert extents[0][0] >= 0 and extents[-1][1] <= V * 3 * max_rows * 7 * 24, what


def test_plans_under_sanitizers(build_dir):
    exe = _build(build_dir, "plan_main_san",
                 ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r, f = _run(exe)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert f["cases"] == CASES and f["violations"] == 0
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_mutant_reports_violations(plan_main):
    """slot: rank r >= 1 one slot too far leaves slot `weight` without an owner (its rows belong
    to nobody) and puts the last rank past the receive buffer, in every case with n > 1."""
    r, f = _run(plan_main, "slot")
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert f["cases"] == CASES
    assert f["cover"] > 0 and f["overlap"] > 0 and f["violations"] > 0
