"""The tables of tests/transmittance_sets.py can tell a right kernel from a wrong one: checked
here on the CPU oracle, with no device.  The GPU tests (tests/test_gpu_transmittance.py) compare
the device with these tables bit for bit; this file shows that both outcomes, the partial
transmittances of glass, the 64-step counter, the 1e-4 exit and the rules that set the query apart
from the occlusion query are all in them."""
import numpy as np
import pytest

import occlusion_sets as oc
import raysets
import transmittance_sets as ts


def _shares(e):
    return float((e == 1.0).mean()), float((e == 0.0).mean())


@pytest.mark.parametrize("name", list(raysets.SCENES))
def test_ray_tables_show_both_outcomes(oracle, name):
    """On every scene at least a quarter of the pairs are fully lit and at least a quarter
    fully blocked, and every value lies in [0, 1]."""
    e = ts.scene_table(name)["expected"]
    one, zero = _shares(e)
    print(f"{name}: {len(e)} pairs, T == 1 {one:.2f}, T == 0 {zero:.2f}")
    assert ((e >= 0.0) & (e <= 1.0)).all()
    assert one >= 0.25 and zero >= 0.25


@pytest.mark.parametrize("name", ["glass", "glass_tri_area"])
def test_glass_tables_hold_partial_transmittance(oracle, name):
    e = ts.scene_table(name)["expected"]
    mid = e[(e > 0.0) & (e < 1.0)]
    print(f"{name}: {len(mid)} pairs with 0 < T < 1, {len(np.unique(mid))} distinct values")
    assert len(mid) >= 300 and len(np.unique(mid)) >= 10


@pytest.mark.parametrize("name", ["c2", "c3", "c4", "mesh"])
def test_light_tables_show_both_outcomes(oracle, name):
    e = ts.light_table(name)["expected"]
    one, zero = int((e == 1.0).sum()), int((e == 0.0).sum())
    print(f"{name}: {e.shape} T == 1 : T == 0 = {one}:{zero}")
    assert one >= 0.15 * e.size and zero >= 0.15 * e.size


@pytest.mark.parametrize("name", ["glass", "glass_tri_area"])
def test_light_tables_of_glass_hold_partial_transmittance(oracle, name):
    e = ts.light_table(name)["expected"]
    mid = int(((e > 0.0) & (e < 1.0)).sum())
    print(f"{name}: {mid} pairs with 0 < T < 1")
    assert mid >= 30


@pytest.mark.parametrize("n", ts.SHELL_COUNTS)
def test_shells_show_the_step_counter(oracle, n):
    """At +inf a ray that crosses 32 shells or more (64 surfaces) never sees the opaque sphere:
    T = 1; one that crosses fewer reaches it: T = 0.  Both happen for both counts."""
    t = ts.crafted_table(f"shells{n}")
    inf = np.flatnonzero(np.isinf(t["dist"]))
    seen = set()
    for k in inf:
        crossed = ts.crossed_shells(n, t["rays"][k])
        want = 1.0 if crossed >= 32 else 0.0
        assert t["expected"][k] == want, (t["rays"][k], crossed)
        seen.add(want)
    assert seen == {0.0, 1.0}


def test_row_shows_the_1e4_exit_and_the_clamp(oracle):
    """Transparency 0.5: the march stops at T = 0.5^14 <= 1e-4, seven spheres in, and never
    reaches the plane — along the axis at either length of d.  Transparencies 0.9 and 1.5: the
    1.5 counts as 1, so the whole row gives 0.9^12 before the opaque plane gives 0."""
    t = ts.crafted_table("row")
    inf = np.isinf(t["dist"]) & (t["index"] < 4)
    assert inf.sum() == 4 and (t["expected"][inf] == 0.5 ** 14).all()
    assert 0.5 ** 14 == 6.103515625e-05
    assert len(np.unique(t["expected"])) >= 14
    c = ts.crafted_table("row_clamp")
    vals = np.unique(c["expected"])
    # every partial value is a product of 0.9s alone, and all twelve of them are met
    want = np.cumprod(np.full(12, 0.9))
    assert np.array_equal(vals[(vals > 0.0) & (vals < 1.0)], np.sort(want))


def test_not_the_occlusion_query(oracle):
    """Glass: pairs that the occlusion query calls occluded (tpos < maxDist) and that still
    transmit light.  plane_at_zero: a closest hit compared with maxDist would call every ray
    blocked by the plane under its origin; the march steps off it."""
    t = ts.scene_table("glass")
    tp = oc.tpos(t["sc"], t["base"])
    with np.errstate(invalid="ignore"):
        occluded = tp[t["index"]] < t["dist"]
    assert (occluded & (t["expected"] > 0.0)).sum() >= 1
    p = ts.crafted_table("plane_at_zero")
    at10 = p["dist"] == 10.0
    assert list(p["expected"][at10]) == [0.0, 0.0, 1.0, 1.0]
    naive = np.zeros(4)      # the plane at t == 0 < 10 is the closest hit of all four rays
    assert not np.array_equal(p["expected"][at10], naive)


def test_light_table_is_the_ray_table_rule(oracle):
    """The light tables' zeros come from two places: skipped lights and blocked shadow rays.
    Both kinds are present on c2, so a kernel that forgets the skips is caught."""
    t = ts.light_table("c2")
    (lpos, _, _), = t["sc"].lights
    _, _, cast = ts.shadow_rays(t["points"], lpos, ts.BIAS)
    e = t["expected"][:, 0]
    assert (~cast).sum() >= 10 and (cast & (e == 0.0)).sum() >= 10 and (cast & (e == 1.0)).sum() >= 10
