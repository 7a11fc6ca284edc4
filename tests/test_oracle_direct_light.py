"""The tables of tests/direct_light_sets.py are right and can tell a right kernel from a wrong
one: checked here on the CPU, with no device.  The restatement of Scene::directLightning is held
against the oracle's TraceRay where the two must agree, the tables are shown to hold every branch
of the light loop, and the host C++ Scene::DirectLightning (examples/direct_light_scenefile
--host-only) is held against the restatement.  The GPU tests (tests/test_gpu_direct_light.py)
compare the device with the same tables."""
import os
import subprocess

import numpy as np
import pytest

import direct_light_sets as dl
from raytracingengine_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "bin", "direct_light_scenefile")


def scatter(s, values):
    """[n_rays, 3]: `values` at the rays that hit, +0.0 elsewhere."""
    out = np.zeros((s["n_rays"], 3), np.float64)
    out[s["index"]] = values[:s["n_hits"]]
    return out


# ------------------------------------------------------------------ the restatement is right
@pytest.mark.parametrize("name", dl.DIRECT_SCENES)
def test_restatement_equals_trace_ray(oracle, name):
    """Every material of these scenes has transparency 0 and specular 0 and there is no area
    light, so TraceRay(ray, 0, bias) = 0 + directLightning * 1.0 at the hit: the restatement's
    radiance equals oracle_trace_rays on the hit rays (==, which takes -0 for +0)."""
    s = dl.scene_set(name)
    assert s["sc"].area_light is None
    assert (s["materials"][:, 4] == 0.0).all() and (s["materials"][:, 5] == 0.0).all()
    ref, _, _ = oracle.trace_rays(s["sc"], s["rays"][s["index"]])
    assert s["n_hits"] == len(ref) >= 300 and not s["pow"].any()
    got = s["radiance"][:s["n_hits"]]
    bad = np.flatnonzero((got != ref).any(axis=1))
    assert not len(bad), (name, len(bad), got[bad[:4]], ref[bad[:4]])
    assert (ref != 0.0).any(axis=1).mean() >= 0.25      # lit points, not a table of zeros


def test_restatement_with_the_specular_term(oracle):
    """Materials with 0 < specular <= 1e-3: directLightning includes the Blinn-Phong term and
    TraceRay casts no reflection ray, so the two still agree — through pow, hence within
    1e-12 * max(1, |ref|) per channel."""
    s = dl.lowspec_set()
    spec = s["materials"][:, 4]
    assert ((spec > 0.0) & (spec <= 1e-3)).mean() >= 0.5
    ref, _, _ = oracle.trace_rays(s["sc"], s["rays"][s["index"]])
    ok = dl.within_bar(s["radiance"], ref)
    err = np.abs(s["radiance"] - ref) / np.maximum(1.0, np.abs(ref))
    print(f"lowspec: {len(ref)} hits, pow at {int(s['pow'].sum())}, max scaled error {err.max():.3e}")
    assert ok.all(), (np.argwhere(~ok)[:4], err.max())
    assert s["pow"].sum() >= 100 and (s["specular"][s["pow"]] != 0.0).any(axis=1).all()
    # the term is in the value: without it the radiance differs
    assert not dl.within_bar(s["materials"][:, :3] * s["diffuse"], ref).all()


# ------------------------------------------------------------------ the tables are not vacuous
@pytest.mark.parametrize("name", dl.LIGHT_SCENES)
def test_tables_hold_skipped_and_cast_pairs(oracle, name):
    s = dl.scene_set(name)
    cast = s["cast"]
    lit = (s["diffuse"] != 0.0).any(axis=1)
    print(f"{name}: {cast.shape} pairs, cast {cast.mean():.2f}, lit points {lit.mean():.2f}")
    assert cast.mean() >= 0.10 and (~cast).mean() >= 0.10
    assert lit.any() and (~lit).any()


def test_tables_hold_the_transmittance_drop(oracle):
    """0 < T <= bias: the light is dropped although its shadow ray arrives (Scene.h:105)."""
    r = dl.row_set()
    T = r["T"][:, 0]
    dropped = r["cast"][:, 0] & (T > 0.0) & (T <= r["bias"])
    kept = r["cast"][:, 0] & (T > r["bias"]) & (T < 1.0)
    print("row: T towards the first light", T)
    assert dropped.sum() >= 2 and kept.sum() >= 2
    # the second light reaches these points, so their diffuse is exactly its term alone
    only_second = dl.expected(_without_first_light(r["sc"]), r["points"], r["materials"])
    assert dl.same_bits(r["diffuse"][dropped], only_second["diffuse"][dropped])
    assert not dl.same_bits(r["diffuse"][kept], only_second["diffuse"][kept])


def _without_first_light(sc):
    import copy
    out = copy.deepcopy(sc)
    del out.lights[0]
    return out


def test_tables_hold_the_specular_gates(oracle):
    """Non-zero specular accumulators on c3 / c4 (with caller-supplied materials: the scenes' own
    have specular 0), and transparent materials whose accumulator stays zero although
    specular > 0 and the point is lit."""
    for name in dl.SPEC_SCENES:
        s = dl.scene_set(name, own_materials=False)
        m = s["materials"]
        nz = (s["specular"] != 0.0).any(axis=1)
        lit = (s["diffuse"] != 0.0).any(axis=1)
        gated = (m[:, 5] > 0.0) & (m[:, 4] > 0.0) & lit
        print(f"{name}: specular != 0 at {int(nz.sum())} of {len(nz)}, gated off at {int(gated.sum())}")
        assert nz.sum() >= 50 and s["pow"].sum() >= nz.sum()
        assert gated.sum() >= 5 and not nz[gated].any()
        assert (lit & (m[:, 4] == 0.0) & ~nz).sum() >= 5
    g = dl.scene_set("glass")
    m = g["materials"]
    lit = (g["diffuse"] != 0.0).any(axis=1)
    gated = (m[:, 5] > 0.0) & (m[:, 4] > 0.0) & lit
    assert gated.sum() >= 1 and not (g["specular"][gated] != 0.0).any()
    assert ((g["specular"] != 0.0).any(axis=1)).sum() >= 1      # the floor's term


# ------------------------------------------------------------------ the host C++ method
@pytest.mark.parametrize("name", ["c2", "glass", "dl_lowspec"])
def test_host_cpp_direct_lightning(oracle, tmp_path, name):
    """Scene::DirectLightning(hit, viewDir, normalIn) on the hits of Scene::IntersectClosestHost,
    through the example's --host-only mode (no device): the restatement's radiance bit for bit
    where pow is not reached, within the bar where it is, +0.0 where a ray misses."""
    build.build_cpp_api()
    s = dl.lowspec_set() if name == "dl_lowspec" else dl.scene_set(name)
    scene = tmp_path / "scene.txt"
    s["sc"].write(scene)
    s["rays"].tofile(tmp_path / "rays.f64")
    subprocess.run([EXE, "--host-only", str(scene), str(tmp_path / "rays.f64"), str(tmp_path)],
                   check=True, capture_output=True, timeout=120)
    assert sorted(p.name for p in tmp_path.glob("*.f64")) == ["rays.f64", "single.f64"]
    single = np.fromfile(tmp_path / "single.f64", np.float64).reshape(-1, 3)
    want = scatter(s, s["radiance"])
    assert single.shape == want.shape
    exact = np.ones(len(want), bool)
    exact[s["index"]] = ~s["pow"][:s["n_hits"]]
    bad = np.flatnonzero((single.view(np.uint64) != want.view(np.uint64)).any(axis=1) & exact)
    assert not len(bad), (name, len(bad), single[bad[:4]], want[bad[:4]])
    assert dl.within_bar(single, want).all()
    if name != "c2":
        assert s["pow"].any()
