"""The drop-in C++20 API (raytracingengine_amd/api: Math.h, Shape.h, Light.h, Scene.h, Image.h)
end to end on the GPU: examples/bin/render_scenefile builds a reference-shaped Scene from a
scene file and calls RenderImage, RenderImageTonemapped, GeneratePixelAt,
GenerateAntiAliasing, CalculatePixelDepth / IntersectClosest, tonemap, tonemapAll and writePPM.
Checked against the C oracle and the reference goldens."""
import os
import subprocess

import numpy as np
import pytest

import tonemap_sets as tm
from raytracingengine_amd.configs import make_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "bin", "render_scenefile")
POW_TOL = 1e-12


def run_api(sc, tmp_path, rays=None):
    scene = tmp_path / "scene.txt"
    sc.write(scene)
    args = [EXE, str(scene), str(tmp_path)]
    if rays is not None:
        rays.astype(np.float64).tofile(tmp_path / "rays.f64")
        args.append(str(tmp_path / "rays.f64"))
    subprocess.run(args, check=True, capture_output=True, timeout=300)
    W, H = sc.camera.width, sc.camera.height
    out = {
        "hdr": np.fromfile(tmp_path / "hdr.f64", np.float64).reshape(H, W, 3),
        "fused": np.fromfile(tmp_path / "fused1.u8", np.uint8).reshape(H, W, 3),
        "tmall": np.fromfile(tmp_path / "tmall.u8", np.uint8).reshape(7, H * W, 3),
        "aces": np.fromfile(tmp_path / "tmaces.u8", np.uint8).reshape(H * W, 3),
        "probe": np.fromfile(tmp_path / "probe.f64", np.float64).reshape(5, 15),
        "stats": tuple(map(int, open(tmp_path / "stats.txt").read().split())),
        "ppm": open(tmp_path / "image.ppm", "rb").read(),
    }
    if rays is not None:
        out["closest"] = np.fromfile(tmp_path / "closest.f64", np.float64).reshape(-1, 9)
    return out


@pytest.mark.parametrize("name", ["c2", "c1", "mirror", "glass", "mesh", "c4"])
def test_cpp_api_matches_oracle(tmp_path, oracle, name):
    sc = make_config(name, 96, 54)
    out = run_api(sc, tmp_path)
    ref, nt, ns = oracle.render(sc)
    assert np.abs(out["hdr"] - ref).max() <= POW_TOL
    assert out["stats"] == (nt, ns)
    exact = np.all(out["hdr"] == ref, axis=-1).reshape(-1)
    assert np.array_equal(out["fused"].reshape(-1, 3)[exact], oracle.tonemap(ref, 1)[exact])
    for op in range(7):   # equal to the oracle's; operator 4 (log, pow) within tonemap_sets' rule
        tm.assert_bytes(out["tmall"][op], out["hdr"], op, f"{name} tonemapAll {op}")
    assert np.array_equal(out["aces"], out["tmall"][6])
    W, H = 96, 54
    assert out["ppm"].startswith(f"P6\n{W} {H}\n255\n".encode())
    assert out["ppm"][len(f"P6\n{W} {H}\n255\n"):] == out["fused"].tobytes()
    probes = [(0, 0), (W - 1, 0), (W // 2, H // 2), (W // 3, 2 * H // 3), (W - 1, H - 1)]
    for (x, y), row in zip(probes, out["probe"]):
        assert np.array_equal(row[0:3], out["hdr"][y, x])      # GeneratePixelAt
        assert np.array_equal(row[3:6], out["hdr"][y, x])      # GenerateAntiAliasing, AA=1
        typ, idx, vals = oracle.closest(sc, oracle.get_ray(sc, x, y))
        assert int(row[6]) == typ
        if typ:
            assert np.array_equal(row[8:15], vals)


def test_cpp_intersect_closest_vs_reference_golden(tmp_path, golden):
    """IntersectClosest through the C++ API reproduces the reference's own HitInfo, including
    the model index it reports for Model hits (Scene.h:251-253)."""
    k = golden["kats"]
    sc = make_config("mesh", 96, 54)
    out = run_api(sc, tmp_path, rays=k["closest_rays"])
    ref = k["closest_out"]
    assert np.array_equal(out["closest"][:, 0], ref[:, 0])
    hit = ref[:, 0] > 0
    assert np.array_equal(out["closest"][hit, 1], ref[hit, 1])
    assert np.array_equal(out["closest"][hit, 2:], ref[hit, 2:])


def test_box_demo_runs(tmp_path):
    exe = os.path.join(ROOT, "examples", "bin", "box_demo")
    res = subprocess.run([exe, "200", "1"], cwd=tmp_path, check=True, capture_output=True,
                         text=True, timeout=300)
    assert "trace" in res.stdout
    for name in ["simple", "reinhard_simple", "reinhard_extended", "reinhard_extended_luminance",
                 "reinhard_jodie", "uncharted2", "aces"]:
        data = (tmp_path / f"{name}.ppm").read_bytes()
        assert data.startswith(b"P6\n200 200\n255\n") and len(data) == 15 + 200 * 200 * 3
