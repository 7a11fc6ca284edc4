"""The fix-up variant's split launch: a frame batch whose frames all have tile lists next to their
class words (rt_shadow_table.hpp, formed by packet_cone_table_kernel) renders its uniform tiles in
packet_uniform_kernel, one wave per list entry, and its general workgroups in
packet_direct_kernel's kFeatSplit twin over the frame's list of them.  Frames are the same bits
either way, so every frame here is rendered with RTAMD_PK_TILE_SPLIT 1 and 0 through the fix-up
(RTAMD_PK_FIX=1) and the marching (=0: never split) variant and compared bit for bit with the C
oracle, doubles and bytes, and with each other; rt_debug_tile_split shows which frames were split.

Each case renders a batch of three moving cameras (first-seen cameras: no lists, one launch),
then the first position three times: the first of those forms the camera's cached table with its
lists (one launch still: the host does not know the counts yet), the others are split, their
grids sized by the lists' counts.  Scenes: the five
kinds of test_gpu_tile_class.py, `all_sky` (no general workgroup: an empty general list) and
`no_uniform` (a sphere over the whole view: an empty uniform list).  Sizes: 64x48, 104x72 (13 x 9
tiles: an odd tile column, so the last workgroup of a row has a wave past the image edge) and
200x120.
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import test_gpu_tile_class as tc
from raytracingengine_amd import capi

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (104, 72), (200, 120)]
BIAS = tc.BIAS
THIRD = (-0.9, 0.3, -27.0)


def all_sky(w, h):
    """A plane and a sphere behind the camera: every tile is a sky tile."""
    sc = tc._scene(w, h)
    sc.add_plane((0.0, 0.0, -100.0), (0.0, 0.0, 1.0), tc.GREY)
    sc.add_sphere((0.0, 0.0, -60.0), 2.0, tc.RED)
    sc.add_light((3.0, 11.0, -12.0), (1.0, 1.0, 1.0), 300.0)
    return sc


def no_uniform(w, h):
    """A sphere over the whole view: every tile has it in its cone mask."""
    sc = tc._floor_wall(tc._scene(w, h))
    sc.add_sphere((0.0, 0.0, 0.0), 23.0, tc.RED)
    sc.add_light((3.0, 11.0, -40.0), (1.0, 1.0, 1.0), 900.0)
    return sc


SCENES = dict(tc.SCENES, all_sky=all_sky, no_uniform=no_uniform)
KINDS = ["below_floor", "horizon", "near_lights", "room", "three_lights", "all_sky", "no_uniform"]


@functools.lru_cache(maxsize=None)
def _reference(kind, size, pos, op):
    """The oracle's frame and its bytes under tonemap `op`, computed once and shared (read-only)."""
    from oracle import pyoracle
    sc = SCENES[kind](*size)
    sc = dataclasses.replace(sc, camera=dataclasses.replace(sc.camera, position=tuple(pos)))
    ref, _, _ = pyoracle.render(sc, max_recursion=10, bias=BIAS)
    ref8 = pyoracle.tonemap(ref, op).reshape(size[1], size[0], 3)
    ref.setflags(write=False)
    ref8.setflags(write=False)
    return ref, ref8


def _split_used(ctx, before):
    return tuple(int(v) for v in np.array(ctx.debug_tile_split()) - before)


def _check(ctx, monkeypatch, kind, size, plan=None, op=1, lists=True):
    plan = plan or {}
    w, h = size
    sc = SCENES[kind](w, h)
    rows = tc._plan_rows(h, plan)
    pos = [tuple(sc.camera.position), tc.SECOND, THIRD]
    refs = [_reference(kind, size, p, op) for p in pos]
    outs = {}
    for fix in ("1", "0"):
        for split in ("1", "0"):
            monkeypatch.setenv("RTAMD_PK_FIX", fix)
            monkeypatch.setenv("RTAMD_PK_TILE_SPLIT", split)
            whole = (0, 0) if fix == "0" else (0, 3)
            halves = (3, 0) if fix == "1" and split == "1" and lists else whole
            ds = ctx.scene(sc)
            try:
                opts = capi.default_opts(tonemap=op, bias=BIAS, flags=capi.RT_FLAG_NO_TILE_ORDER,
                                         **plan)
                for rnd, cams in enumerate((pos, [pos[0]] * 3, [pos[0]] * 3, [pos[0]] * 3)):
                    before = np.array(ctx.debug_tile_split())
                    got, got8 = tc._batch(ctx, ds, ds.cameras(np.array(cams, np.float64)), opts,
                                          len(rows), w)
                    want = halves if rnd >= 2 else whole
                    assert _split_used(ctx, before) == want, (fix, split, rnd)
                    for f, p in enumerate(cams):
                        ref, ref8 = refs[pos.index(p)]
                        assert np.array_equal(got[f], ref[rows]), (fix, split, rnd, f)
                        assert np.array_equal(got8[f], ref8[rows]), (fix, split, rnd, f)
                    outs[(fix, split, rnd)] = (got, got8)
                # one-frame launches never take the fix-up variant, so they are never split
                before = np.array(ctx.debug_tile_split())
                out = ds.render(hdr64=True, tonemap=op, opts=opts)
                assert _split_used(ctx, before) == (0, 0)
                assert np.array_equal(out["hdr64"], refs[0][0][rows])
                assert np.array_equal(out["ldr"], refs[0][1][rows])
            finally:
                ds.close()
    for rnd in range(4):  # the split launch's frames are the single launch's, bit for bit
        a, a8 = outs[("1", "1", rnd)]
        b, b8 = outs[("1", "0", rnd)]
        assert np.array_equal(a, b) and np.array_equal(a8, b8), rnd


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", KINDS)
def test_split_frames_are_the_oracles(ctx, monkeypatch, kind, size):
    _check(ctx, monkeypatch, kind, size)


@pytest.mark.parametrize("size", SIZES[1:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_block_cyclic_rows_are_the_oracles_rows(ctx, monkeypatch, size):
    _check(ctx, monkeypatch, "room", size, plan=tc.PLANS["3x3"])


def test_another_tonemap_than_reinhard(ctx, monkeypatch):
    _check(ctx, monkeypatch, "near_lights", (104, 72), op=2)


def test_two_wave_rows_per_workgroup_are_never_split(ctx, monkeypatch):
    """Workgroups of two wave rows (WGY = 2) belong to packet images past 16 KiB, more than 64
    spheres: such scenes get no class words and no fix-up variant, so nothing is split; 64
    spheres, the most the fix-up variant renders, have cone masks only and stay whole too."""
    _check(ctx, monkeypatch, "spheres64", (104, 72), lists=False)


def test_moving_batches_on_two_streams_wrap_the_table_ring(ctx, monkeypatch):
    """Seven batches of three first-seen cameras alternate between two streams without waiting
    and wrap the four-entry ring of images and tables.  A batch of first-seen cameras forms no
    lists and is never split (its counts would not be known to the host: both grids would cover
    every tile, which measured slower); every frame is the frame rendered with the switch off
    (afterwards, one batch at a time) and, for the first and the last batch, the oracle's."""
    w, h = 104, 72
    sc = SCENES["room"](w, h)
    monkeypatch.setenv("RTAMD_PK_FIX", "1")
    base = np.array(sc.camera.position)
    batches = [[tuple(base + (0.01 * (3 * b + f + 1), -0.005 * f, 0.02 * b)) for f in range(3)]
               for b in range(7)]
    opts = capi.default_opts(tonemap=1, bias=BIAS, flags=capi.RT_FLAG_NO_TILE_ORDER)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    ds = ctx.scene(sc)
    try:
        monkeypatch.setenv("RTAMD_PK_TILE_SPLIT", "1")
        before = np.array(ctx.debug_tile_split())
        outs = []
        for b, pos in enumerate(batches):
            ctx.set_stream(streams[b % 2].cuda_stream)
            h64 = torch.full((3 * h * w * 3,), -1.0, dtype=torch.float64, device="cuda")
            l8 = torch.zeros(3 * h * w * 3, dtype=torch.uint8, device="cuda")
            ds.render_batch(ds.cameras(np.array(pos, np.float64)), h64.data_ptr(), None,
                            l8.data_ptr(), opts)
            outs.append((h64, l8))
        torch.cuda.synchronize()
        ctx.set_stream(None)
        assert _split_used(ctx, before) == (0, 21)
        got = [(a.cpu().numpy().reshape(3, h, w, 3), b8.cpu().numpy().reshape(3, h, w, 3))
               for a, b8 in outs]
    finally:
        ctx.set_stream(None)
        ds.close()
    monkeypatch.setenv("RTAMD_PK_TILE_SPLIT", "0")
    ds = ctx.scene(sc)
    try:
        for b, pos in enumerate(batches):
            before = np.array(ctx.debug_tile_split())
            one, one8 = tc._batch(ctx, ds, ds.cameras(np.array(pos, np.float64)), opts, h, w)
            assert _split_used(ctx, before) == (0, 3)
            assert np.array_equal(got[b][0], one) and np.array_equal(got[b][1], one8), b
    finally:
        ds.close()
    for b in (0, 6):
        for f, p in enumerate(batches[b]):
            ref, ref8 = _reference("room", (w, h), p, 1)
            assert np.array_equal(got[b][0][f], ref) and np.array_equal(got[b][1][f], ref8), (b, f)


def test_a_launch_with_a_tile_order_stays_whole(ctx, monkeypatch):
    """The default flags: the first two batches are whole (a first-seen camera, then the launch
    that forms its table), the third batch of a camera records its wave durations (the general
    variant: no fix-up variant, so neither count moves), the fourth builds the costliest-first
    order and dispatches by it — an ordered launch is one launch, (0, n), and forms no lists —
    and later ones are split again when the order kernel found the costs narrow, else stay
    whole.  Every frame is the oracle's."""
    w, h = 104, 72
    sc = SCENES["room"](w, h)
    monkeypatch.setenv("RTAMD_PK_FIX", "1")
    monkeypatch.setenv("RTAMD_PK_TILE_SPLIT", "1")
    pos = tuple(sc.camera.position)
    ref, ref8 = _reference("room", (w, h), pos, 1)
    opts = capi.default_opts(tonemap=1, bias=BIAS)
    ds = ctx.scene(sc)
    try:
        used = []
        for rnd in range(6):
            before = np.array(ctx.debug_tile_split())
            got, got8 = tc._batch(ctx, ds, ds.cameras(np.array([pos] * 3, np.float64)), opts, h, w)
            used.append(_split_used(ctx, before))
            for f in range(3):
                assert np.array_equal(got[f], ref) and np.array_equal(got8[f], ref8), (rnd, f)
        assert used[:4] == [(0, 3), (0, 3), (0, 0), (0, 3)], used
        assert all(u in ((3, 0), (0, 3)) for u in used[4:]), used
    finally:
        ds.close()
