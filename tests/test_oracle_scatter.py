"""The tables of tests/scatter_sets.py are right and can tell a right kernel from a wrong one:
checked here on the CPU, with no device.  The numpy restatement of one TraceRay level, applied
level by level, is held against the oracle's TraceRay bit for bit; the tables are shown to hold
every branch of the level (refraction, reflection, total internal reflection, back faces); and no
present-or-absent decision of a table lies near its threshold.  The GPU tests
(tests/test_gpu_scatter.py) compare the device with the same tables."""
import numpy as np
import pytest

import direct_light_sets as dl
import raysets
import scatter_sets as ss

# scene, maxRecursion
RECOMPOSE = (("glass", 3), ("mirror", 4), ("c1", 3), ("c2", 2), ("mesh", 3), ("glass", 0))


def assert_canonical(got, ref, what):
    a, b = dl.canonical_bits(got), dl.canonical_bits(ref)
    bad = np.flatnonzero((a != b).any(axis=1))
    assert a.shape == b.shape and not len(bad), (what, len(bad), bad[:6], got[bad[:3]], ref[bad[:3]])


@pytest.mark.parametrize("name,depth", RECOMPOSE)
def test_levels_recompose_trace_ray(oracle, name, depth):
    """TraceRay(ray, 0) == value + TraceRay(refraction child, 1) * fw + TraceRay(reflection
    child, 1) * rw, applied down to maxRecursion = depth: the oracle's TraceRay, bit for bit."""
    sc = raysets.scene(name)
    rays, _ = raysets.rayset(sc)
    ref, _, _ = oracle.trace_rays(sc, rays, max_recursion=depth, use_area_light=False)
    got = ss.compose(sc, rays, depth)
    assert_canonical(got, ref, (name, depth))
    if depth == 0:
        assert_canonical(got, ss.sky(rays), "all sky")


@pytest.mark.parametrize("name", ("glass", "mirror"))
def test_levels_recompose_nonfinite_rays(oracle, name):
    sc = raysets.scene(name)
    rays = raysets.nonfinite_rays(sc)
    ref, _, _ = oracle.trace_rays(sc, rays, max_recursion=2, use_area_light=False)
    assert_canonical(ss.compose(sc, rays, 2), ref, name)


def test_coverage_floors():
    """The level-0 tables hold every branch often enough for the device test to mean something."""
    c = {name: ss.counts(ss.scene_set(name)) for name in ss.SCENES}
    for name, k in c.items():
        print(name, k)
    g = c["glass"]
    assert g["refract"] >= 50 and g["reflect"] >= 200 and g["tir"] >= 10 and g["back"] >= 30, g
    assert c["mirror"]["reflect"] >= 500, c["mirror"]
    assert c["mesh"]["reflect"] >= 50, c["mesh"]
    for name in ("c2", "sph300"):
        assert c[name]["refract"] == 0 and c[name]["reflect"] == 0 and c[name]["hits"] >= 300, c[name]
    assert c["glass_tri_area"]["tir"] >= 5, c["glass_tri_area"]


@pytest.mark.parametrize("name", ss.SCENES)
def test_threshold_margin(name):
    """No present-or-absent decision lies within 1e-9 of its threshold (|rw - bias| on hits,
    |length(refract) - bias| on transparent hits), so the 1e-12 bar on the Fresnel pow can never
    flip a flag: a condition on the inputs."""
    t = ss.scene_set(name)
    hit = (t["flags"] & ss.HIT) != 0
    rw, ln = t["rw_margin"][hit], t["len_margin"][hit]
    print(f"{name}: min |rw - bias| {rw.min():.3e}, min |length(refract) - bias| {ln.min():.3e}")
    assert (rw > 1e-9).all() and (ln > 1e-9).all()


def test_area_light_is_left_out_of_the_table():
    """glass_tri_area keeps its area light; its table is the one of the scene without it."""
    t = ss.scene_set("glass_tri_area")
    assert t["sc"].area_light is not None
    bare = ss.level(ss.without_area_light(t["sc"]), t["rays"])
    for k in ss.OUTPUTS:
        assert np.array_equal(t[k], bare[k]), k
