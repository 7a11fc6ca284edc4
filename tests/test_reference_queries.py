"""The expected tables of the batch queries against the compiled reference
(tests/golden/query_tables.npz, made by tests/golden/make_golden.py --queries): what
Scene::IntersectAnyBefore, computeTransmittance, directLightning, TraceRay at several recursion
limits and IntersectClosest of the unmodified reference answer to the inputs of
tests/occlusion_sets.py, transmittance_sets.py, direct_light_sets.py, scatter_sets.py and
raysets.py.  The GPU suite holds the kernels to those tables; here the tables themselves, and the
oracle where it is the table, are held to the reference.

Bar: bit for bit, as tests/test_oracle_golden.py (the same IEEE operations in the same order and
glibc's pow on both sides), a NaN equal to a NaN.  Every test checks the hashes of its inputs
first, so a generator that drifted fails with its own message.

The specular accumulator is read from the reference through a material of colour 0, whose
0 * diffuseAccumulation is NaN where that accumulator is not finite (some non-finite points):
there the reference gives no specular to compare, element by element.

That the fixture is not vacuous is asserted on the fixture itself: on what the reference said."""
import importlib.util
import os

import numpy as np
import pytest

import direct_light_sets as dl
import raysets
import reference_query_sets as rq
import scatter_sets as sset
import transmittance_sets as ts

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF_HARNESS = os.path.join(os.path.dirname(GOLDEN), os.pardir, "oracle", "_ref", "ref_harness")
BIAS = rq.BIAS
OCC_MIN_SHARE = 0.20      # tests/test_oracle_occlusion.py MIN_SHARE


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, rq.FIXTURE)))


@pytest.fixture(scope="module")
def case(oracle):
    """Every case by key, made once (the tables behind them are cached by their modules)."""
    return {c["key"]: c for c in rq.cases()}


def bad_rows(got, ref):
    a, b = rq.canonical_bits(got), rq.canonical_bits(ref)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))


def assert_bits(got, ref, what, detail=None):
    bad = bad_rows(got, ref)
    assert not len(bad), (what, len(bad), bad[:8], np.asarray(got)[bad[:4]], np.asarray(ref)[bad[:4]],
                          None if detail is None else detail(bad[:4]))


def test_fixture_holds_every_case_and_nothing_else(golden, case):
    keys = {k for k in golden if k != "bias" and not k.endswith("#in")}
    assert keys == set(case)
    assert float(golden["bias"]) == BIAS
    assert os.path.getsize(os.path.join(GOLDEN, rq.FIXTURE)) < 1_000_000


# ------------------------------------------------------------------ IntersectAnyBefore
def occ_params():
    return ([("scene", n) for n in rq.OCC_SCENES] + [("crafted", n) for n in raysets.CRAFTED]
            + [("nonfinite", n) for n in rq.OCC_NONFINITE])


@pytest.mark.parametrize("kind,name", occ_params())
def test_occlusion_tables(golden, case, kind, name):
    key = f"occ/{kind}/{name}"
    rq.check_inputs(golden, case[key])
    t = rq.occlusion_table(kind, name)
    ref = golden[key]
    assert ref.dtype == np.uint8 and ((ref == 0) | (ref == 1)).all()
    bad = np.flatnonzero(t["expected"] != ref.astype(bool))
    assert not len(bad), (key, len(bad), bad[:8], t["rays"][bad[:4]], t["dist"][bad[:4]],
                          t["tpos"][t["index"][bad[:4]]])
    # the share tests/test_oracle_occlusion.py asks of the table, here of the reference's answers
    assert OCC_MIN_SHARE <= ref.mean() <= 1.0 - OCC_MIN_SHARE, (key, ref.mean())


def test_plane_at_zero(golden, case):
    """The plane under the origins is at t = 0: `0 < t < maxDist` does not count it, `t < maxDist`
    would (all four rays true at every positive distance)."""
    rq.check_inputs(golden, case["occ/plane_at_zero"])
    t = rq.plane_at_zero()
    ref = golden["occ/plane_at_zero"].astype(bool).reshape(len(rq.PLANE_AT_ZERO_DIST), 4)
    assert rq.PLANE_AT_ZERO_DIST[1] == np.inf
    assert list(ref[1]) == [True, True, False, False]
    assert np.array_equal(t["expected"].reshape(ref.shape), ref)
    assert list(ref[2]) == [False, True, False, False]     # t = 4 < 4 is false; |d| = 2: t = 2
    assert list(ref[3]) == [True, True, False, False]


# ------------------------------------------------------------------ computeTransmittance
def tr_params():
    return ([("scene", n) for n in rq.TR_SCENES] + [("grid", n) for n in ts.BVH_GRIDS]
            + [("nonfinite", n) for n in rq.TR_NONFINITE] + [("crafted", n) for n in ts.CRAFTED])


@pytest.mark.parametrize("kind,name", tr_params())
def test_transmittance_tables(golden, case, kind, name):
    key = f"tr/{kind}/{name}"
    rq.check_inputs(golden, case[key])
    t = rq.transmittance_table(kind, name)
    ref = golden[key]
    assert_bits(t["expected"], ref, key, lambda b: (t["rays"][b], t["dist"][b]))
    if kind == "scene":   # the shares tests/test_oracle_transmittance.py asks of the table
        assert (ref == 0.0).mean() >= 0.25 and (ref == 1.0).mean() >= 0.25, key


def test_transmittance_crafted_rows_say_what_they_are_built_for(golden):
    """On the reference's answers: the T <= 1e-4 exit leaves 0.5^14 (not 0.5^13, above 1e-4, and
    not 0.5^15 or less), the clamp of transparency 1.5 to 1 leaves every power of 0.9 up to the
    twelfth (six spheres of 0.9, two surfaces each), and more than 32 shells use up the 64 steps
    before the opaque sphere is seen."""
    row = golden["tr/crafted/row"]
    assert (row == 0.5 ** 14).any() and not ((row > 0.0) & (row < 0.5 ** 14)).any()
    clamp = golden["tr/crafted/row_clamp"]
    powers = [0.9]
    for _ in range(11):
        powers.append(powers[-1] * 0.9)
    for p in powers:
        assert (clamp == p).any(), p
    assert clamp.max() <= 1.0 and not ((clamp > 0.0) & (clamp < powers[-1])).any()
    t70, t40 = ts.crafted_table("shells70"), ts.crafted_table("shells40")
    g70, g40 = golden["tr/crafted/shells70"], golden["tr/crafted/shells40"]
    far = np.isposinf(t70["dist"])
    deep = np.array([ts.crossed_shells(70, r) > 32 for r in t70["rays"]])
    assert (far & deep).any() and (g70[far & deep] == 1.0).all()
    far40 = np.isposinf(t40["dist"])
    through = np.array([0 < ts.crossed_shells(40, r) <= 31 for r in t40["rays"]])
    assert (far40 & through).any() and (g40[far40 & through] == 0.0).all()


@pytest.mark.parametrize("name", rq.TR_SHADOW_SCENES)
def test_shadow_rays_of_the_light_tables(golden, case, name):
    """light_table's transmittance where a shadow ray is cast, light by light."""
    t = ts.light_table(name)
    seen = []
    for l in range(len(t["sc"].lights)):
        key = f"tr/shadow/{name}/{l}"
        rq.check_inputs(golden, case[key])
        s = rq.shadow_case(name, l)
        assert_bits(s["expected"], golden[key], key, lambda b: (s["rays"][b], s["dist"][b]))
        assert (np.asarray(t["expected"])[~s["cast"], l] == 0.0).all()
        seen.append(golden[key])
    seen = np.concatenate(seen)
    assert (seen == 0.0).any() and (seen == 1.0).any(), name
    if name == "glass":
        assert ((seen > 0.0) & (seen < 1.0)).any()


# ------------------------------------------------------------------ directLightning
def assert_direct(e, ref, what):
    """e: a table of direct_light_sets.expected; ref [n,9]: the reference's radiance, diffuse and
    specular accumulators."""
    assert_bits(e["radiance"], ref[:, 0:3], (what, "radiance"))
    assert_bits(e["diffuse"], ref[:, 3:6], (what, "diffuse"))
    spec = np.array(e["specular"])
    readable = np.isfinite(ref[:, 3:6])
    assert readable.mean() >= 0.5, what
    assert_bits(np.where(readable, spec, 0.0), np.where(readable, ref[:, 6:9], 0.0),
                (what, "specular"))


@pytest.mark.parametrize("suffix,kind,name", rq.direct_sets())
def test_direct_light_tables(golden, case, suffix, kind, name):
    key = f"dl/{suffix}"
    rq.check_inputs(golden, case[key])
    s = rq.direct_set(kind, name)
    ref = golden[key]
    assert_direct(s, ref, key)
    if kind != "nonfinite":
        assert np.isfinite(ref).all(), key
    if kind in ("spec", "row", "lowspec", "bias_edge"):   # the Blinn-Phong term is in the answer
        assert (ref[:, 6:9] != 0.0).any() and s["pow"].any(), key


def test_row_set_drops_the_first_light_from_the_fifth_point_on(golden):
    """One-light goldens of dl_row: the point behind k spheres sees the first light at
    T = 0.5^(2k), above the bias up to k = 4; from k = 5 on T <= bias and the reference adds
    nothing (Scene.h:105)."""
    lit = (golden["dl/light/row/0"] != 0.0).any(axis=1)
    assert list(lit) == [True] * 5 + [False] * (len(lit) - 5)
    # the second light, unobstructed, stays: the drop is the first light's transmittance
    assert (golden["dl/light/row/1"] != 0.0).any(axis=1)[5:].all()


def test_bias_edge_drops_the_light_at_a_transmittance_of_exactly_the_bias(golden):
    """dl_bias_edge, one light: T is the bias under the first triangle, one unit in the last place
    above it under the second, one below under the third.  The reference drops the light at
    T <= bias (Scene.h:105): lit under the second triangle only, in the diffuse and in the
    specular accumulator."""
    ref = golden["dl/bias_edge"]
    k = dl.BIAS_EDGE_POINTS
    for cols in (slice(3, 6), slice(6, 9)):
        lit = (ref[:, cols] != 0.0).all(axis=1)
        dark = (ref[:, cols] == 0.0).all(axis=1)
        assert list(lit) == [False] * k + [True] * k + [False] * k
        assert list(dark) == [True] * k + [False] * k + [True] * k
    T = np.asarray(dl.bias_edge_set()["T"])[:, 0]
    assert list(T) == [t for t in dl.bias_edge_transparencies() for _ in range(k)]


@pytest.mark.parametrize("name", rq.DL_PER_LIGHT)
def test_one_light_goldens_pin_the_skips(golden, case, name):
    """The reference with one light only: its diffuse accumulator is non-zero exactly where the
    table says the shadow ray is cast and T > bias, and it is that light's term of the table."""
    s = rq.per_light_set(name)
    cast, T = np.asarray(s["cast"]), np.asarray(s["T"])
    skipped = lit = total = 0
    summed = np.zeros((len(s["points"]), 3))
    for l in range(len(s["sc"].lights)):
        key = f"dl/light/{name}/{l}"
        rq.check_inputs(golden, case[key])
        ref = golden[key]
        assert np.isfinite(ref).all()
        on = (ref != 0.0).any(axis=1)
        want = cast[:, l] & (T[:, l] > s["bias"])
        bad = np.flatnonzero(on != want)
        assert not len(bad), (key, bad[:8], s["points"][bad[:4]], T[bad[:4], l])
        assert (T[~cast[:, l], l] == 0.0).all()
        skipped += int((~on).sum())   # on the golden: a `continue`, or T <= bias
        lit += int(on.sum())
        total += len(on)
        summed = summed + ref          # the reference's own order of the sum over the lights
    assert skipped >= 0.15 * total and lit >= 0.15 * total, (name, skipped, lit, total)
    assert_bits(summed, s["diffuse"], (name, "sum of the one-light diffuse accumulators"))


# ------------------------------------------------------------------ TraceRay levels
@pytest.mark.parametrize("name", rq.TRACE_SCENES)
def test_trace_at_every_recursion_limit(golden, case, oracle, name):
    sc = raysets.scene(name)
    rays, _ = raysets.rayset(sc)
    for d in rq.TRACE_DEPTHS:
        key = f"trace/{name}/{d}"
        rq.check_inputs(golden, case[key])
        got, _, _ = oracle.trace_rays(sc, rays, max_recursion=d, bias=BIAS)
        assert_bits(got, golden[key], key, lambda b: rays[b])
    assert_bits(sset.sky(rays), golden[f"trace/{name}/0"], (name, "the sky at limit 0"))
    assert not rq.same(golden[f"trace/{name}/0"], golden[f"trace/{name}/1"])
    if name != "c2":       # children matter: the limits differ from one another
        assert not rq.same(golden[f"trace/{name}/1"], golden[f"trace/{name}/2"])
        assert not rq.same(golden[f"trace/{name}/2"], golden[f"trace/{name}/3"])
    else:
        assert rq.same(golden["trace/c2/1"], golden["trace/c2/16"])
    ten = dict(np.load(os.path.join(GOLDEN, "ray_queries.npz")))[f"{name}_trace"]
    if name in ("mirror", "glass"):
        assert not rq.same(golden[f"trace/{name}/16"], ten)


@pytest.mark.parametrize("name", rq.COMPOSE_SCENES)
@pytest.mark.parametrize("depth", rq.COMPOSE_DEPTHS)
def test_compose_of_levels_is_the_reference(golden, case, oracle, name, depth):
    """scatter_sets.compose — `level` applied level by level — is the reference's TraceRay with
    maxRecursion = depth: the only handle the reference gives on one TraceRay level."""
    key = f"trace/{name}/{depth}"
    rq.check_inputs(golden, case[key])
    sc = raysets.scene(name)
    rays, _ = raysets.rayset(sc)
    assert_bits(sset.compose(sc, rays, depth), golden[key], key, lambda b: rays[b])


# ------------------------------------------------------------------ IntersectClosest
def assert_closest(got, ref, sc, what):
    """The oracle's nine doubles against the reference's; a Model's triangles report the model's
    index in the reference, so the index is compared on the other rows."""
    assert got.shape == ref.shape
    assert np.array_equal(got[:, 0], ref[:, 0]), (what, np.flatnonzero(got[:, 0] != ref[:, 0])[:8])
    assert_bits(got[:, 2:], ref[:, 2:], what)
    rows = np.ones(len(ref), bool) if not sc.models else got[:, 0] != 3
    assert np.array_equal(got[rows, 1], ref[rows, 1]), what


@pytest.mark.parametrize("name", list(raysets.CRAFTED))
def test_closest_on_crafted_sets(golden, case, oracle, name):
    key = f"closest/crafted/{name}"
    rq.check_inputs(golden, case[key])
    sc, rays, side = raysets.CRAFTED[name]()
    ref = golden[key]
    assert_closest(oracle.closest_rays(sc, rays), ref, sc, key)
    if name in raysets.THRESHOLD_SETS:     # both sides of the threshold, in the reference's answers
        assert 0.20 <= side(ref).mean() <= 0.80, (key, side(ref).mean())


@pytest.mark.parametrize("name", rq.NONFINITE_RAY_SCENES)
def test_nonfinite_rays(golden, case, oracle, name):
    sc = raysets.scene(name)
    rays = raysets.nonfinite_rays(sc)
    key = f"closest/nonfinite/{name}"
    rq.check_inputs(golden, case[key])
    assert_closest(oracle.closest_rays(sc, rays), golden[key], sc, key)
    key = f"trace/nonfinite/{name}"
    rq.check_inputs(golden, case[key])
    ref = golden[key]
    assert_bits(oracle.trace_rays(sc, rays, bias=BIAS)[0], ref, key, lambda b: rays[b])
    assert np.isfinite(ref).all(axis=1).sum() >= 5
    if name == "glass":
        assert np.isnan(ref).any()


# ------------------------------------------------------------------ regeneration
@pytest.mark.skipif(not os.path.exists(REF_HARNESS),
                    reason="oracle/_ref/ref_harness is not built (needs the reference sources)")
def test_fixture_regenerates(golden, oracle, tmp_path):
    """make_golden.py --queries into a temporary directory gives the committed fixture."""
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLDEN, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    new = dict(np.load(mg.queries_golden(str(tmp_path))))
    assert set(new) == set(golden)
    for k, v in golden.items():
        if k.endswith("#in"):
            assert list(new[k]) == list(v), k
        else:
            assert new[k].dtype == v.dtype and rq.same(new[k].astype(np.float64),
                                                        v.astype(np.float64)), k
