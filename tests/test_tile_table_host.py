"""The tile table's description (csrc/rt_tile_table.hpp: TileTabContents, TileTabLayout and the
list counts' packing) pinned to literals: tests/tile_table/table_main.cpp, a stand-alone program
with its own main, built here with g++.  It holds the offsets of two small tables (8 tiles in 4
workgroups with two lights, 6 tiles in 3 workgroups with one) written out by hand from the
documented layout, the sizes of the tables that end early, the closure rules of the contents,
the distinctness of their key words and the round trip of the counts, "not yet" included.
CPU only.
"""
import os
import re
import subprocess

from host_programs import build

SRC = "tests/tile_table/table_main.cpp"


def _run(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    print(r.stdout, r.stderr[-2000:])
    return r, {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", r.stdout)}


def test_layout_contents_and_counts(tmp_path):
    r, f = _run(build(tmp_path, "table_main", SRC, [], oracle=False))
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    assert f["failed"] == 0
    assert f["checks"] == 52  # every expect() of the program ran


def test_host_program_under_sanitizers(tmp_path):
    """The same stand-alone program with AddressSanitizer and UBSan."""
    exe = build(tmp_path, "table_main_san", SRC,
                ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                 "-fno-omit-frame-pointer"], oracle=False)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r, f = _run(exe, env)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    assert f["failed"] == 0
