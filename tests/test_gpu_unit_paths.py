"""GPU parity of the three paths of unit() (rt_device.hpp) inside one wave.

unit() returns a vector of length exactly 1 as it is, divides through the shared-reciprocal core
when every component is at least 2^-900 in magnitude, and through three literal divisions
otherwise.  The fallback is a branch of its own (tests/test_isa_unit_branch.py); these frames
make single waves mix lanes of all three paths at the camera-ray site and check every pixel
against the C oracle.

Frames are 16x8 — one 128-thread workgroup of the packet kernel, two 8x8 waves, wave 1 starting
at x = 8 — with focal = 1, so the camera ray of pixel (x, y) is unit((x - 8) - cx, (4 - y) - cy, 1):
  * camera (0, 0, z): column 8 has a zero x component, row 4 a zero y component (fallback), and
    the centre pixel's ray is (0, 0, 1): length exactly 1 and two zero components;
  * camera (0.25, 0.125, z): no zero component, only the core runs;
  * camera (2^-950, 0, z): column 8 gets the non-zero component -2^-950, below the core's
    2^-900 numerator gate — the fallback with a non-zero numerator (its square underflows, so
    the centre ray still has length exactly 1).
One 13x5 frame (camera (0.5, 0.5, z): zero components in column 7 and row 2, the centre ray
(0, 0, 1)) adds the lanes past the image edge, which trace a clamped in-image ray.
"""
import numpy as np
import pytest
import torch

from raytracingengine_amd import capi
from raytracingengine_amd.scene import Camera, Material, SceneData

pytestmark = pytest.mark.gpu

CHAIN_TOL = 1e-12  # reflection chains call pow (Blinn-Phong): the bar of tests/test_gpu_parity.py
Z = -3.0
CASES = {"axis": (16, 8, (0.0, 0.0, Z)), "core_only": (16, 8, (0.25, 0.125, Z)),
         "tiny_x": (16, 8, (2.0 ** -950, 0.0, Z)), "edge_13x5": (13, 5, (0.5, 0.5, Z))}
PATHS = ["march", "fixup", "generic", "box_chain"]


def _scene(case, mirror):
    w, h, pos = CASES[case]
    sc = SceneData(Camera(pos, 1.0, w, h, 0.0, 200.0, 1), name=f"unit_{case}")
    sc.add_sphere((0.0, 0.0, 2.0), 4.0, Material((0.8, 0.4, 0.3)))
    floor = Material((0.7, 0.8, 0.9), shininess=32.0, specular=0.25) if mirror \
        else Material((0.7, 0.8, 0.9))
    sc.add_plane((0.0, -5.0, 0.0), (0.0, 1.0, 0.0), floor)
    sc.add_light((3.0, 6.0, -4.0), (1.0, 1.0, 1.0), 60.0)
    return sc


@pytest.fixture(scope="module")
def references(oracle):
    """{(case, mirror): (scene, oracle HDR, oracle Reinhard bytes)}, rendered once."""
    out = {}
    for case in CASES:
        for mirror in (False, True):
            sc = _scene(case, mirror)
            ref, _, _ = oracle.render(sc)
            out[case, mirror] = (sc, ref, oracle.tonemap(ref, 1).reshape(ref.shape))
    return out


def test_cases_reach_every_path():
    """The cameras do what the module docstring says (Camera::getRay's arithmetic in numpy)."""
    def rays(case):
        w, h, (cx, cy, _) = CASES[case]
        x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
        v = np.stack([(x - w / 2.0) - cx, (h / 2.0 - y) - cy, np.ones_like(x)], -1)
        with np.errstate(under="ignore"):
            l = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
        small = (np.abs(v) < 2.0 ** -900).any(-1)
        return v, l == 1.0, small & (l != 1.0), ~small & (l != 1.0)
    v, one, fallback, core = rays("axis")
    assert one.sum() == 1 and one[4, 8] and fallback[:, 8].sum() == 7 and fallback[4].sum() == 15
    assert core[:, 8:].any() and fallback[:, 8:].any()  # wave 1 mixes them
    v, one, fallback, core = rays("core_only")
    assert core.all()
    v, one, fallback, core = rays("tiny_x")
    # (2^-1900 underflows: the centre ray's length is still exactly 1)
    assert (v[:, 8, 0] == -2.0 ** -950).all() and fallback[:, 8].sum() == 7 and one[4, 8]
    v, one, fallback, core = rays("edge_13x5")
    assert one[2, 7] and fallback[:, 7].sum() == 4 and fallback[2].sum() == 12


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", list(CASES))
def test_unit_paths_vs_oracle(ctx, references, monkeypatch, case, path):
    """Every pixel of the frame against the oracle: HDR bits and Reinhard bytes equal through the
    marching packet variant, the fix-up variant (RTAMD_PK_FIX=1, a batch of 2 frames) and the
    generic kernel; within 1e-12 through box_chain_kernel (a mirror floor: reflection chains)."""
    sc, ref, ref8 = references[case, path == "box_chain"]
    w, h = sc.camera.width, sc.camera.height
    ds = ctx.scene(sc)
    try:
        if path == "fixup":
            monkeypatch.setenv("RTAMD_PK_FIX", "1")
            n = 2
            H64 = torch.full((n * h * w * 3,), -1.0, dtype=torch.float64, device="cuda")
            L8 = torch.zeros(n * h * w * 3, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ds.render_batch(ds.cameras(np.repeat(ds.camera["position"], n, axis=0)),
                            H64.data_ptr(), None, L8.data_ptr(), capi.default_opts(tonemap=1))
            ctx.synchronize()
            frames = list(zip(H64.cpu().numpy().reshape(n, h, w, 3),
                              L8.cpu().numpy().reshape(n, h, w, 3)))
        else:
            monkeypatch.setenv("RTAMD_PK_FIX", "0")
            flags = capi.RT_FLAG_GENERIC_KERNEL if path == "generic" else 0
            out = ds.render(hdr64=True, tonemap=1, flags=flags)
            frames = [(out["hdr64"], out["ldr"])]
    finally:
        ds.close()
    for hdr, ldr in frames:
        if path == "box_chain":
            assert np.abs(hdr - ref).max() <= CHAIN_TOL
            same = np.all(hdr == ref, axis=-1)
            assert np.array_equal(ldr[same], ref8[same])
        else:
            assert np.array_equal(hdr.view(np.int64), ref.view(np.int64)), \
                np.argwhere(hdr.view(np.int64) != ref.view(np.int64))[:8]
            assert np.array_equal(ldr, ref8)
