"""The byte-boundary table of tests/tonemap_sets.py against the compiled reference
(tests/golden/tonemap_edges.npz, made by tests/golden/make_golden.py --tonemap-edges): pixels
within a few ulps of every value at which a tonemap operator's byte changes, where an operator that
is one ulp off writes another byte.  Here the oracle (bytes of all seven operators, operator 4's
curve) and the table itself are held to what the reference answered; tests/test_gpu_tonemap.py
holds the device to the same table.

Bar: bit for bit, as tests/test_oracle_golden.py, a NaN equal to a NaN.

The table's sensitivity is tested as well: numpy restatements of ACES, Uncharted2 and
Reinhard-extended must give the fixture's bytes, and four variants of them that are wrong by an
ulp or so — each matches the 1024 random pixels of kats.npz on every byte — must not."""
import importlib.util
import os

import numpy as np
import pytest

import tonemap_sets as tm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF_HARNESS = os.path.join(os.path.dirname(GOLDEN), os.pardir, "oracle", "_ref", "ref_harness")


@pytest.fixture(scope="module")
def edges():
    return dict(np.load(os.path.join(GOLDEN, tm.FIXTURE)))


@pytest.fixture(scope="module")
def px(oracle, edges):
    """The table's pixels, rebuilt from the stored thresholds."""
    return tm.inputs(edges["thresholds"])


def test_thresholds_and_inputs_rebuild(oracle, edges, px):
    thr = tm.thresholds()
    assert tm.same(thr, edges["thresholds"])
    assert tm.sha(px) == str(edges["inputs_sha256"]) == tm.sha(tm.inputs())
    reach = (~np.isnan(thr)).sum(axis=1)
    assert list(reach) == [255, 251, 255, 255, 26, 255, 255]
    n = int(reach.sum()) * len(tm.ULPS)
    assert px.shape == (2 * n + len(tm.SPECIALS) ** 3, 3)
    assert np.array_equal(px[:n, 0].view(np.int64), px[:n, 1].view(np.int64))      # gray
    assert np.isnan(px[2 * n:]).any() and np.isinf(px[2 * n:]).any()               # specials


def test_thresholds_are_where_the_reference_byte_changes(edges, px):
    """On the fixture itself: at each threshold's gray pixel the reference's byte of that operator
    is k, and one ulp below it is k - 1."""
    thr = edges["thresholds"]
    row = 0
    for op in range(tm.N_OPS):
        ks = np.flatnonzero(~np.isnan(thr[op])) + 1
        at = row + np.arange(len(ks)) * len(tm.ULPS) + tm.ULPS.index(0)
        assert np.array_equal(px[at, 0], thr[op][ks - 1])
        assert np.array_equal(edges["bytes"][op, at, 0], ks), op
        assert np.array_equal(edges["bytes"][op, at - 1, 0], ks - 1), op
        row += len(ks) * len(tm.ULPS)


def test_oracle_bytes_and_curve_are_the_reference(oracle, edges, px):
    ref = edges["bytes"]
    assert ref.shape == (8, len(px), 3)
    for op in range(tm.N_OPS):
        got = oracle.tonemap(px, op)
        bad = np.flatnonzero((got != ref[op]).any(axis=1))
        assert not len(bad), (tm.po_name(op), len(bad), px[bad[:4]], got[bad[:4]], ref[op][bad[:4]])
    assert np.array_equal(ref[7], ref[6])      # tonemap() is the ACES operator
    assert tm.same(oracle.curves(px, tm.JODIE), edges["jodie_curve"])
    assert np.isnan(edges["jodie_curve"]).any() and np.isfinite(edges["jodie_curve"]).any()


def test_oracle_curves_are_kats_curves(oracle, golden):
    """oracle_tonemap_curves on the 1024 pixels of kats.npz: the reference's curves of all seven
    operators (ref_harness curves), bit for bit."""
    k = golden["kats"]
    for op in range(tm.N_OPS):
        assert tm.same(oracle.curves(k["tonemap_in"], op), k["tonemap_curves"][op]), op
    assert np.isnan(k["tonemap_curves"]).any()


@pytest.mark.skipif(not os.path.exists(REF_HARNESS),
                    reason="oracle/_ref/ref_harness is not built (needs the reference sources)")
def test_fixture_regenerates(oracle, edges, tmp_path):
    """make_golden.py --tonemap-edges into a temporary directory gives the committed fixture."""
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLDEN, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    path = mg.tonemap_edges_golden(str(tmp_path))
    new = dict(np.load(path))
    assert set(new) == set(edges)
    assert str(new["inputs_sha256"]) == str(edges["inputs_sha256"])
    assert np.array_equal(new["bytes"], edges["bytes"])
    assert tm.same(new["thresholds"], edges["thresholds"])
    assert tm.same(new["jodie_curve"], edges["jodie_curve"])
    assert os.path.getsize(path) <= 1_000_000


# ------------------------------------------------------------------ the table's sensitivity
def f32(x):
    """A float literal of the reference: rounded to float, then promoted."""
    return np.float64(np.float32(x))


def smax(a, b):     # std::max(a, b): a NaN in b is dropped
    return np.where(a < b, b, a)


def smin(a, b):     # std::min(a, b)
    return np.where(b < a, b, a)


def to_color(v):
    with np.errstate(invalid="ignore"):
        return (smin(1.0, smax(0.0, v)) * 255.0).astype(np.uint8)


def aces(c, lit=f32):
    v = c * lit(0.6)
    a, b, cc, d, e = lit(2.51), lit(0.03), lit(2.43), lit(0.59), lit(0.14)
    return smin(1.0, smax(0.0, (v * (v * a + b)) / (v * (v * cc + d) + e)))


def uncharted2(c, float_products=True, reciprocal=True):
    A, B, C, D, E, F = (np.float32(x) for x in (0.15, 0.50, 0.10, 0.20, 0.02, 0.30))
    if float_products:
        CB, DE, DF, EF = (np.float64(x) for x in (C * B, D * E, D * F, E / F))
    else:
        CB, DE, DF, EF = (np.float64(C) * np.float64(B), np.float64(D) * np.float64(E),
                          np.float64(D) * np.float64(F), np.float64(E) / np.float64(F))
    A, B = np.float64(A), np.float64(B)

    def partial(x):
        return (x * (x * A + CB) + DE) / (x * (x * A + B) + DF) - EF
    cur = partial(c * 2.0)
    white = partial(np.float64(11.2))
    return cur * (1.0 / white) if reciprocal else cur / white


def reinhard_extended(c, divide=True):
    inner = c / 25.0 if divide else c * (1.0 / 25.0)
    return (c * (inner + 1.0)) / (c + 1.0)


GOOD = {"aces": (6, aces), "uncharted2": (5, uncharted2), "reinhard_extended": (2, reinhard_extended)}
BROKEN = {
    "aces: constants as doubles, not float-rounded": (6, lambda c: aces(c, lit=np.float64)),
    "uncharted2: C*B, D*E, D*F, E/F formed in double": (5, lambda c: uncharted2(c, float_products=False)),
    "uncharted2: divided by the white scale": (5, lambda c: uncharted2(c, reciprocal=False)),
    "reinhard_extended: c * (1/25) for c / 25": (2, lambda c: reinhard_extended(c, divide=False)),
}


def _bytes(fn, c):
    with np.errstate(all="ignore"):
        return to_color(fn(np.asarray(c, np.float64)))


@pytest.mark.parametrize("name", list(GOOD))
def test_restated_operators_give_the_table(edges, px, golden, name):
    op, fn = GOOD[name]
    assert np.array_equal(_bytes(fn, px), edges["bytes"][op])
    assert np.array_equal(_bytes(fn, golden["kats"]["tonemap_in"]), golden["kats"]["tonemap_bytes"][op])


@pytest.mark.parametrize("name", list(BROKEN))
def test_broken_operators_are_caught(edges, px, golden, name):
    """Each variant is invisible to the 1024 random pixels and differs on the boundary table: a
    table that lost its sensitivity fails here."""
    op, fn = BROKEN[name]
    k = golden["kats"]
    assert np.array_equal(_bytes(fn, k["tonemap_in"]), k["tonemap_bytes"][op])
    differ = int((_bytes(fn, px) != edges["bytes"][op]).sum())
    print(f"{name}: {differ} of {px.size} bytes differ")
    assert differ >= 1
