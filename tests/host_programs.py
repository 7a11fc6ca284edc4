"""What the tests of the stand-alone host check programs (tests/*/..._main.cpp) share: the build
of one such program against the C oracle, and the frame file the programs read.
"""
from __future__ import annotations

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(d, name, src, extra, oracle=True, sources=(), cxx_extra=()):
    """Compiles `src` (a path under the repository root) into d/name, with the C oracle unless
    the program does not call it, and returns the executable's path; `extra` goes to both
    compilers (sanitizer flags).  `sources`: further C++ files of the repository to compile in
    (the library's host code under test); `cxx_extra`: flags they need, for g++ alone."""
    objs = []
    if oracle:
        objs.append(str(d / f"rt_oracle_{name}.o"))
        subprocess.run(["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-fopenmp", *extra,
                        f"-I{ROOT}/oracle", "-c", f"{ROOT}/oracle/rt_oracle.c", "-o", objs[0]],
                       check=True)
    exe = str(d / name)
    subprocess.run(["g++", "-std=c++20", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                    *extra, *cxx_extra, f"-I{ROOT}/raytracingengine_amd/csrc", f"-I{ROOT}/oracle",
                    f"{ROOT}/{src}", *(f"{ROOT}/{s}" for s in sources), *objs, "-o", exe,
                    "-fopenmp", "-lm"], check=True)
    return exe


def write_frame_file(path, scene, bias):
    """One frame of `scene` from its own camera, as tests/host_frame.hpp's read_frame reads it."""
    def hexes(vals):
        return " ".join(float(v).hex() for v in vals)

    cam = scene.camera
    with open(path, "w") as fh:
        fh.write(f"{cam.width} {cam.height} {hexes((*cam.position, cam.focal, bias))} "
                 f"{len(scene.spheres)} {len(scene.planes)} {len(scene.lights)}\n")
        for s in scene.spheres:
            fh.write(hexes((*s[0], s[1])) + "\n")
        for p in scene.planes:
            fh.write(hexes((*p[0], *p[1])) + "\n")
        for l in scene.lights:
            fh.write(hexes(l[0]) + "\n")
