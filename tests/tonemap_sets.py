"""The inputs of the tonemap byte tests and the rule their bytes are held to: one table for
tests/golden/make_golden.py --tonemap-edges (which records what oracle/_ref/ref_harness answers
into tests/golden/tonemap_edges.npz), tests/test_tonemap_edges.py (which holds the oracle and the
table's own sensitivity to those answers on the CPU) and tests/test_gpu_tonemap.py (which holds the
device's stand-alone kernel, resolve and every fused store to them).

A byte is trunc(clamp(curve(c)) * 255), so an operator that is one ulp off shows only where
curve * 255 stands within an ulp of an integer: random pixels never do.  The table puts pixels
there.  Per operator and byte k = 1..255, `thresholds` bisects, over the doubles' integer
representation in [0, G_MAX], for the smallest gray value whose oracle byte is >= k (operator 1
reaches 251 of them below G_MAX, operator 4 reaches 26; an unreachable one is NaN).  The bisection
only chooses where to look: the expected bytes are the reference's at the exact inputs, so nothing
assumes that an operator is monotone.  `inputs` is then, in this order,

    gray      every threshold of every operator at the ulp offsets ULPS, as (g, g, g)
    mixed     the same values as triples: each operator's block permuted three times with a fixed
              seed, one permutation per channel, so a per-channel operator sees a value next to
              one of its own thresholds in every channel, and operators 3 and 4 leave the gray axis
    specials  every triple of SPECIALS: +-0, 5e-324, 1e-300, 1e6, 2^53, 1e300, +-inf, NaN, -1, -0.5

No special is left out: the reference's toColor clamps through std::min(1, std::max(0, v)), which
turns a NaN into 0 and every other double into [0, 1] before the cast to a byte, so the cast never
sees a NaN or an out-of-range value (RaytracingEngine.cpp:70-76, 113-121).
"""
from __future__ import annotations

import functools
import hashlib
import itertools

import numpy as np

from oracle import pyoracle as po

FIXTURE = "tonemap_edges.npz"
N_OPS = 7
G_MAX = 64.0
ULPS = tuple(range(-4, 5))
SEED = 20261020
SPECIALS = (0.0, -0.0, 5e-324, 1e-300, 1e6, 2.0 ** 53, 1e300, np.inf, -np.inf, np.nan, -1.0, -0.5)
JODIE = 4
JODIE_ULPS = 8.0     # assert_bytes' bar for operator 4


def _gray_bytes(g: np.ndarray, op: int) -> np.ndarray:
    return po.tonemap(np.repeat(g[:, None], 3, axis=1), op)[:, 0].astype(np.int64)


@functools.lru_cache(maxsize=None)
def thresholds() -> np.ndarray:
    """float64 [7, 255]: per operator and byte k = 1..255 the smallest gray value in [0, G_MAX]
    whose oracle byte is >= k, NaN where G_MAX itself stays below k."""
    k = np.arange(1, 256, dtype=np.int64)
    out = np.full((N_OPS, 255), np.nan)
    top = np.array([G_MAX]).view(np.int64)[0]
    for op in range(N_OPS):
        reach = _gray_bytes(np.full(255, G_MAX), op) >= k
        assert (_gray_bytes(np.zeros(255), op) < k).all()
        lo = np.zeros(255, np.int64)          # byte(lo) < k
        hi = np.full(255, top, np.int64)      # byte(hi) >= k where reachable
        while (hi - lo > 1).any():
            mid = lo + (hi - lo) // 2
            up = _gray_bytes(mid.view(np.float64), op) >= k
            hi = np.where(up, mid, hi)
            lo = np.where(up, lo, mid)
        out[op, reach] = hi.view(np.float64)[reach]
    out.setflags(write=False)
    return out


def inputs(thr: np.ndarray | None = None) -> np.ndarray:
    """The table's pixels, float64 [n, 3], from the thresholds (default: thresholds())."""
    thr = thresholds() if thr is None else np.asarray(thr, np.float64)
    rng = np.random.default_rng(SEED)
    gray, mixed = [], []
    for op in range(N_OPS):
        t = thr[op][~np.isnan(thr[op])]
        bits = t.view(np.int64)[:, None] + np.asarray(ULPS, np.int64)[None, :]
        v = np.maximum(bits, 0).reshape(-1).view(np.float64)
        gray.append(np.repeat(v[:, None], 3, axis=1))
        mixed.append(np.stack([rng.permutation(v) for _ in range(3)], axis=1))
    specials = np.array(list(itertools.product(SPECIALS, repeat=3)), np.float64)
    return np.ascontiguousarray(np.concatenate(gray + mixed + [specials]))


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).hexdigest()


def same(a, b) -> bool:
    """Bit for bit, every NaN equal to every NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64))
                                              | (np.isnan(a) & np.isnan(b))))


# ------------------------------------------------------------------ the rule for the bytes
def boundary_ulps(curve: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """For curve values before toColor: (the integer nearest to y*255, the distance of y*255
    from it in ulps of y*255), y the value clamped as toColor clamps it (a NaN is 0)."""
    y = np.asarray(curve, np.float64)
    y = np.where(0.0 < y, y, 0.0)
    y = np.where(y < 1.0, y, 1.0)
    p = y * 255.0
    r = np.rint(p)
    return r, np.abs(p - r) / np.spacing(np.maximum(p, np.finfo(np.float64).tiny))


def check_bytes(got, ref, op: int, curve=None, what="") -> float:
    """Hold device bytes `got` to reference bytes `ref` of operator `op`.

    Every operator but 4 is IEEE +, *, / in the reference's order (division is correctly rounded
    on the device, tests/test_gpu_parity.py test_device_libm): the arrays must be equal.

    Operator 4, Reinhard-Jodie, calls log twice and pow once.  There a byte may differ from the
    reference's only if it differs by exactly 1 and the reference curve value y (`curve`, the
    value before toColor), clamped to [0, 1], has y*255 within JODIE_ULPS = 8 ulps of y*255 of the
    integer that separates the two bytes.  The 8 is derived, not measured: device log and pow are
    each within 1 ulp of glibc's (test_device_libm), reinhardJodie and change_luminance make three
    libm calls and five roundings, which is about 6 ulps on y, rounded up.

    Measured on an MI355X (tests/test_gpu_tonemap.py prints it): the largest distance among the
    differing bytes is 1 ulp.  On the boundary table 3 of the 88992 bytes differ from
    tonemap_kernel and from resolve at one sample, 6 after resolve's division of a sum by 3; in
    the rendered 96x54 and 128x72 frames of that module no byte differs.

    Returns the largest distance in ulps among the differing bytes (0.0 when none differs)."""
    got = np.asarray(got).reshape(-1)
    ref = np.asarray(ref).reshape(-1)
    assert got.shape == ref.shape and got.dtype == np.uint8 and ref.dtype == np.uint8, \
        (what, got.shape, ref.shape, got.dtype)
    bad = np.flatnonzero(got != ref)
    if op != JODIE:
        assert not len(bad), (what, po_name(op), len(bad), bad[:8] // 3, got[bad[:8]], ref[bad[:8]])
        return 0.0
    if not len(bad):
        return 0.0
    g, r = got[bad].astype(np.int64), ref[bad].astype(np.int64)
    edge, dist = boundary_ulps(np.asarray(curve, np.float64).reshape(-1)[bad])
    ok = (np.abs(g - r) == 1) & (edge == np.maximum(g, r)) & (dist <= JODIE_ULPS)
    worst = float(dist.max())
    print(f"{what or 'bytes'}: operator 4 differs on {len(bad)} of {got.size} bytes, largest "
          f"distance from a byte boundary {worst:.3g} ulps")
    assert ok.all(), (what, "operator 4 outside the rule", int((~ok).sum()), bad[~ok][:8] // 3,
                      g[~ok][:8], r[~ok][:8], dist[~ok][:8])
    return worst


def assert_bytes(got, hdr, op: int, what="") -> float:
    """check_bytes against the oracle at `hdr` (float64 [..., 3]): pyoracle.tonemap(hdr, op), and
    for operator 4 pyoracle.curves(hdr, 4).  The oracle is the reference on the boundary table
    (tests/test_tonemap_edges.py)."""
    hdr = np.ascontiguousarray(hdr, np.float64).reshape(-1, 3)
    return check_bytes(got, po.tonemap(hdr, op), op,
                       po.curves(hdr, JODIE) if op == JODIE else None, what)


def po_name(op: int) -> str:
    return ("simple", "reinhard_simple", "reinhard_extended", "reinhard_extended_luminance",
            "reinhard_jodie", "uncharted2", "aces")[op]
