"""ctypes binding of ``include/rt_capi.h`` (the HIP library ``librtamd.so``).

This is plumbing for the bench and the parity tests: every call goes straight to the C-ABI.
There is no CPU fallback — if the library or a gfx950 device is missing, the calls raise.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import NamedTuple

import numpy as np

from .scene import AREA_LIGHT_DTYPE, SceneData

HERE = os.path.dirname(os.path.abspath(__file__))
# RTAMD_LIB overrides the library path (A/B builds in tools/); default: the in-tree build.
LIB_PATH = os.environ.get("RTAMD_LIB", os.path.join(HERE, "librtamd.so"))

(RT_OK, RT_ERR_INVALID_ARG, RT_ERR_HIP, RT_ERR_OOM, RT_ERR_UNSUPPORTED, RT_ERR_NO_DEVICE,
 RT_ERR_RCCL) = range(7)
STATUS_NAMES = {0: "RT_OK", 1: "RT_ERR_INVALID_ARG", 2: "RT_ERR_HIP", 3: "RT_ERR_OOM",
                4: "RT_ERR_UNSUPPORTED", 5: "RT_ERR_NO_DEVICE", 6: "RT_ERR_RCCL"}

TONEMAP_NONE = -1
TONEMAPS = ["simple", "reinhard_simple", "reinhard_extended", "reinhard_extended_luminance",
            "reinhard_jodie", "uncharted2", "aces"]
TONEMAP_ALL = 7
RT_FLAG_COUNT_RAYS = 0x1
RT_FLAG_TIME_KERNEL = 0x2
RT_FLAG_GENERIC_KERNEL = 0x4
RT_FLAG_NO_BVH = 0x8
RT_FLAG_PIPELINE = 0x10
RT_FLAG_NO_TILE_ORDER = 0x20
RT_FLAG_NO_SAMPLE_PARALLEL = 0x40
RT_OUT_HDR64, RT_OUT_HDR32, RT_OUT_LDR = 0x1, 0x2, 0x4
RT_COMM_ID_BYTES = 128
# G-buffer outputs (rt_capi.h RT_GB_*)
GB_DEPTH = 0x01
GB_DEPTH_NORM = 0x02
GB_NORMAL = 0x04
GB_PRIM = 0x08
GB_ALBEDO = 0x10
GB_ALL = 0x1F
# direct-lighting outputs (rt_capi.h RT_DL_*), each float64 [n, 3]
DL_RADIANCE = 0x1
DL_DIFFUSE = 0x2
DL_SPECULAR = 0x4
DL_ALL = 0x7
DL_OUTPUTS = [("radiance", DL_RADIANCE), ("diffuse", DL_DIFFUSE), ("specular", DL_SPECULAR)]
# scatter outputs (rt_capi.h RT_SC_*)
SC_VALUE = 0x01
SC_REFRACT = 0x02
SC_REFLECT = 0x04
SC_WEIGHTS = 0x08
SC_FLAGS = 0x10
SC_ALL = 0x1F
# per output, in bit order: name (the key of DeviceScene.scatter's dict and the field of
# rt_scatter_out), bit, element type, elements per ray (0: a flat [n] array)
SC_OUTPUTS = [("value", SC_VALUE, np.float64, 3), ("refract_rays", SC_REFRACT, np.float64, 6),
              ("reflect_rays", SC_REFLECT, np.float64, 6), ("weights", SC_WEIGHTS, np.float64, 2),
              ("flags", SC_FLAGS, np.uint8, 0)]
# closest-hit outputs (rt_capi.h RT_CH_*)
CH_T = 0x01
CH_PRIM = 0x02
CH_NORMAL = 0x04
CH_POINT = 0x08
CH_MATERIAL = 0x10
CH_ALL = 0x1F
# per output, in bit order: name (the key of DeviceScene.closest's dict and the field of
# rt_closest_out), bit, element type, elements per ray (0: a flat [n] array)
CH_OUTPUTS = [("t", CH_T, np.float64, 0), ("prim", CH_PRIM, np.int32, 2),
              ("normal", CH_NORMAL, np.float64, 3), ("point", CH_POINT, np.float64, 3),
              ("material", CH_MATERIAL, np.float64, 7)]
# per output, in bit order: name (the key of DeviceScene.gbuffer's dict and the field of
# rt_gbuffer), bit, element type, elements per pixel
GB_OUTPUTS = [("depth", GB_DEPTH, np.float64, 1), ("depth_norm", GB_DEPTH_NORM, np.float32, 1),
              ("normal", GB_NORMAL, np.float64, 3), ("prim", GB_PRIM, np.int32, 2),
              ("albedo", GB_ALBEDO, np.float32, 3)]

# Every symbol include/rt_capi.h declares (checked by tests/test_capi_symbols.py).
EXPORTED = [
    "rt_last_error", "rt_build_info", "rt_device_count", "rt_render_opts_default", "rt_context_create",
    "rt_context_destroy", "rt_context_set_stream", "rt_context_synchronize", "rt_scene_create",
    "rt_scene_destroy", "rt_scene_set_area_light", "rt_render", "rt_render_device",
    "rt_render_multi", "rt_comm_unique_id", "rt_comm_create", "rt_comm_create_all",
    "rt_comm_create_local", "rt_comm_destroy", "rt_comm_info", "rt_comm_set_root_weight",
    "rt_comm_create_ex", "rt_comm_set_timeout", "rt_render_gather", "rt_render_gather_all",
    "rt_comm_timing", "rt_comm_synchronize", "rt_debug_assemble_rows", "rt_debug_tile_order",
    "rt_stats_read", "rt_stats_reset", "rt_trace_rays", "rt_intersect_rays", "rt_tonemap",
    "rt_debug_f64_ops", "rt_debug_vec_ops", "rt_queue_create", "rt_queue_destroy",
    "rt_queue_submit", "rt_queue_wait", "rt_queue_synchronize", "rt_render_batch",
    "rt_render_gather_batch", "rt_render_gather_all_batch", "rt_gbuffer", "rt_gbuffer_device",
    "rt_debug_cone_table",
    "rt_debug_shadow_table",
    "rt_debug_tile_class",
    "rt_debug_plane_clear",
    "rt_debug_tile_split",
    "rt_debug_tile_shadowed", "rt_debug_fixup_count",
    "rt_occluded_rays", "rt_occluded_rays_device",
    "rt_transmittance_rays", "rt_transmittance_rays_device",
    "rt_light_transmittance", "rt_light_transmittance_device",
    "rt_direct_light", "rt_direct_light_device",
    "rt_direct_light_rays", "rt_direct_light_rays_device",
    "rt_scatter_rays", "rt_scatter_rays_device",
    "rt_light_transmittance_keyed", "rt_light_transmittance_keyed_device",
    "rt_direct_light_keyed", "rt_direct_light_keyed_device",
    "rt_direct_light_rays_keyed", "rt_direct_light_rays_keyed_device",
    "rt_scatter_rays_keyed", "rt_scatter_rays_keyed_device",
    "rt_camera_rays", "rt_camera_rays_device",
    "rt_closest_rays", "rt_closest_rays_device",
    "rt_trace_rays_device",
    "rt_accumulate_samples", "rt_accumulate_samples_device",
    "rt_resolve", "rt_resolve_device",
    "rt_accumulate_adaptive", "rt_accumulate_adaptive_device",
    "rt_resolve_counts", "rt_resolve_counts_device", "rt_debug_adaptive_listed",
]


class RtError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {msg}")
        self.status = status


class SceneDesc(ctypes.Structure):
    _fields_ = [
        ("spheres", ctypes.c_void_p), ("n_spheres", ctypes.c_int32),
        ("planes", ctypes.c_void_p), ("n_planes", ctypes.c_int32),
        ("triangles", ctypes.c_void_p), ("n_triangles", ctypes.c_int32),
        ("lights", ctypes.c_void_p), ("n_lights", ctypes.c_int32),
    ]


class RenderOpts(ctypes.Structure):
    _fields_ = [
        ("max_recursion", ctypes.c_int32), ("tonemap", ctypes.c_int32),
        ("bias", ctypes.c_double), ("seed", ctypes.c_uint64),
        ("row_begin", ctypes.c_uint32), ("row_end", ctypes.c_uint32),
        ("flags", ctypes.c_int32), ("row_block", ctypes.c_uint16), ("row_cycle", ctypes.c_uint16),
    ]


class Stats(ctypes.Structure):
    _fields_ = [
        ("trace_rays", ctypes.c_uint64), ("shadow_rays", ctypes.c_uint64),
        ("kernel_ms", ctypes.c_double), ("launches", ctypes.c_uint64),
    ]


class GBufferPtrs(ctypes.Structure):
    """struct rt_gbuffer: one pointer per output (those of outputs not requested are ignored)."""
    _fields_ = [(name, ctypes.c_void_p) for name, _, _, _ in GB_OUTPUTS]


def gbuffer_layout(outputs: int, width: int, rows: int, frames: int | None = None) -> dict:
    """{name: (shape, dtype)} of the requested G-buffer outputs: [frames,] rows, width[, k]
    (frames None: a single frame without the leading axis).  Pure shape logic, no device."""
    if outputs == 0 or outputs & ~GB_ALL:
        raise ValueError(f"G-buffer outputs {outputs:#x}: no output or an unknown bit")
    lead = () if frames is None else (int(frames),)
    return {name: (lead + (rows, width) + ((k,) if k > 1 else ()), np.dtype(dt))
            for name, bit, dt, k in GB_OUTPUTS if outputs & bit}


class DirectLightPtrs(ctypes.Structure):
    """struct rt_direct_light_out: one pointer per output, in RT_DL_* bit order."""
    _fields_ = [(name, ctypes.c_void_p) for name, _ in DL_OUTPUTS]


def material_rows(materials, n: int) -> np.ndarray:
    """`materials` of the direct-light queries as float64 [1, 7] or [n, 7] rows of rt_material's
    layout {r, g, b, shininess, specular, transparency, refractive_index}: a scene.Material, a
    7-tuple, or an [n, 7] array."""
    if hasattr(materials, "as_tuple"):
        c, *rest = materials.as_tuple()
        materials = (*c, *rest)
    m = np.ascontiguousarray(materials, np.float64)
    if m.ndim == 1:
        m = m.reshape(1, -1)
    if m.ndim != 2 or m.shape[1] != 7 or m.shape[0] not in (1, n):
        raise ValueError("materials: a Material, seven values, or an [n, 7] array")
    return m


class ScatterPtrs(ctypes.Structure):
    """struct rt_scatter_out: one pointer per output, in RT_SC_* bit order."""
    _fields_ = [(name, ctypes.c_void_p) for name, *_ in SC_OUTPUTS]


class ClosestPtrs(ctypes.Structure):
    """struct rt_closest_out: one pointer per output, in RT_CH_* bit order."""
    _fields_ = [(name, ctypes.c_void_p) for name, *_ in CH_OUTPUTS]


class AreaKeysRec(ctypes.Structure):
    """struct rt_area_keys."""
    _fields_ = [("pixel", ctypes.c_void_p), ("sample", ctypes.c_uint32),
                ("depth", ctypes.c_uint32)]


class AreaKeys:
    """The keys of the area light's draws for a batch (rt_area_keys): `pixel` one key per element
    or None (element i draws with pixel = i, as trace_rays), `sample` the AA sample index and
    `depth` the recursion depth of the batch.  pixel on the host: anything
    np.asarray(..., np.uint64) takes, of length n; on the device: a contiguous torch.int64 tensor
    of n elements on the context's device, its bits read as uint64."""

    def __init__(self, pixel=None, sample: int = 0, depth: int = 0):
        self.pixel, self.sample, self.depth = pixel, int(sample), int(depth)

    def at_depth(self, depth: int, pixel=None) -> "AreaKeys":
        return AreaKeys(self.pixel if pixel is None else pixel, self.sample, depth)

    def _host(self, n: int):
        """(the record, the array it points into) for a host entry of n elements."""
        px = None
        if self.pixel is not None:
            px = np.ascontiguousarray(np.asarray(self.pixel, np.uint64).reshape(-1))
            if len(px) != n:
                raise ValueError("area_keys.pixel: n keys")
        ptr = None if px is None or n == 0 else px.ctypes.data
        return AreaKeysRec(ptr, self.sample, self.depth), px

    def _device(self, n: int, dev):
        """The record for a _device entry of n elements on `dev`."""
        if self.pixel is None:
            return AreaKeysRec(None, self.sample, self.depth)
        import torch
        if not torch.is_tensor(self.pixel):
            raise ValueError("area_keys.pixel: a contiguous int64 tensor on the context's device")
        if _checked_input(self.pixel, dev, torch.int64, 1, "area_keys.pixel") != n:
            raise ValueError("area_keys.pixel: n keys")
        return AreaKeysRec(self.pixel.data_ptr() if n else None, self.sample, self.depth)


def _call_level(query: str, args, area_keys, n: int, dev=None) -> None:
    """One call of a per-level query: the entry `query` itself, or with area_keys its _keyed
    sibling with the keys' record after the sibling's arguments.  dev: the device of a _device
    entry's tensors; None: the host entry."""
    form = "" if dev is None else "_device"
    if area_keys is None:
        _check(getattr(_lib, query + form)(*args))
        return
    rec, _keep = area_keys._host(n) if dev is None else (area_keys._device(n, dev), None)
    _check(getattr(_lib, query + "_keyed" + form)(*args, ctypes.byref(rec)))


# The records of selectable outputs by the prefix of their bits: the rows (name, bit, element
# type, elements per item), the ctypes record and all the bits.  DL_OUTPUTS keeps its two columns
# for its users; every direct-light output is float64 [n, 3].
_RECORDS = {kind: (rows, record, sum(r[1] for r in rows)) for kind, rows, record in (
    ("DL", [(name, bit, np.float64, 3) for name, bit in DL_OUTPUTS], DirectLightPtrs),
    ("SC", SC_OUTPUTS, ScatterPtrs), ("CH", CH_OUTPUTS, ClosestPtrs))}


_TORCH_DTYPES = {}   # numpy element type -> torch dtype, filled as _outputs meets them


def _mask_check(kind: str, outputs: int):
    if outputs == 0 or outputs & ~_RECORDS[kind][2]:
        raise ValueError(f"outputs: a non-empty combination of {kind}_* bits")


def _dl_check(outputs: int):
    _mask_check("DL", outputs)


def _sc_check(outputs: int):
    _mask_check("SC", outputs)


def _ch_check(outputs: int):
    _mask_check("CH", outputs)


def _host_rows(a, k: int):
    """`a` as a contiguous float64 [n, k] array, and n."""
    a = np.ascontiguousarray(a, np.float64).reshape(-1, k)
    return a, a.shape[0]


def _checked_input(t, dev, dtype, k: int, name: str) -> int:
    """n of the input tensor `t` of n*k elements: contiguous, of `dtype`, on `dev`."""
    if t.dtype != dtype or t.device != dev or not t.is_contiguous():
        raise ValueError(f"{name}: a contiguous {str(dtype).split('.')[-1]} tensor on the "
                         "context's device")
    n = t.numel() // k
    if t.numel() != k * n:
        raise ValueError(f"{name}: n*{k} elements")
    return n


def _out_tensor(t, dev, dtype, shape, name: str = "out", need: str = "n"):
    """The output tensor `t` as it is, or for None a new one of `shape`: contiguous, of `dtype`,
    on `dev`, of at least prod(shape) elements (`need` in the message)."""
    if t is None:
        import torch
        return torch.empty(shape, dtype=dtype, device=dev)
    if (t.dtype != dtype or t.device != dev or t.numel() < math.prod(shape)
            or not t.is_contiguous()):
        raise ValueError(f"{name}: a contiguous {str(dtype).split('.')[-1]} tensor of at least "
                         f"{need} elements on the device")
    return t


def _outputs(kind: str, outputs: int, n: int, dev=None, out=None):
    """({name: array} of the outputs the `kind`_* bits of `outputs` request for n items, in bit
    order; the ctypes record of their pointers).  dev None: new numpy arrays; else torch tensors
    on `dev`, those `out` holds by name (checked as _out_tensor checks one) or new ones.  A
    requested output's pointer is never NULL, an empty array's included."""
    _mask_check(kind, outputs)
    rows, record, _ = _RECORDS[kind]
    if dev is None:
        res = {name: np.empty((n, k) if k else (n,), dt)
               for name, bit, dt, k in rows if outputs & bit}
        return res, record(**{k: (v.ctypes.data or 8) for k, v in res.items()})
    import torch
    res, ptr = {}, {}
    for name, bit, dt, k in rows:
        if not outputs & bit:
            continue
        tdt = _TORCH_DTYPES.get(dt) or _TORCH_DTYPES.setdefault(dt, getattr(torch, dt.__name__))
        t = None if out is None else out.get(name)
        if t is None:
            t = torch.empty((n, k) if k else (n,), dtype=tdt, device=dev)
        elif (t.dtype != tdt or t.device != dev or t.numel() < max(k, 1) * n
              or not t.is_contiguous()):
            raise ValueError(f"out[{name!r}]: a contiguous {dt.__name__} tensor of at least "
                             f"n*{max(k, 1)} elements on the device")
        res[name] = t
        ptr[name] = t.data_ptr() or 8
    return res, record(**ptr)


def _max_dist_tensor(max_dist, n: int, dev):
    """max_dist of the ray queries as a float64 [n] tensor on `dev`: a scalar is expanded there."""
    import torch
    if not torch.is_tensor(max_dist):
        max_dist = torch.full((n,), float(max_dist), dtype=torch.float64, device=dev)
        # filled on torch's current stream, read on the context's
        torch.cuda.current_stream(dev).synchronize()
    if (max_dist.dtype != torch.float64 or max_dist.device != dev or max_dist.numel() != n
            or not max_dist.is_contiguous()):
        raise ValueError("max_dist: a scalar or a contiguous float64 [n] tensor on the device")
    return max_dist


class GatherTiming(ctypes.Structure):
    _fields_ = [
        ("render_ms", ctypes.c_double), ("gather_ms", ctypes.c_double),
        ("assemble_ms", ctypes.c_double), ("frames", ctypes.c_uint64),
        ("rows", ctypes.c_uint32), ("max_rows", ctypes.c_uint32),
    ]


_lib = None


def load_library(path: str = LIB_PATH):
    """Load librtamd.so; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        # One HIP runtime per process: torch ships its own libamdhip64.so.7; loading it first
        # makes librtamd.so's NEEDED entry bind to that copy instead of /opt/rocm's.
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
            " (hipcc --offload-arch=gfx950). The renderer has no CPU fallback.")
    L = ctypes.CDLL(path)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    L.rt_last_error.restype = ctypes.c_char_p
    if hasattr(L, "rt_build_info") or "RTAMD_LIB" not in os.environ:
        L.rt_build_info.restype = ctypes.c_char_p
        L.rt_build_info.argtypes = []
    L.rt_device_count.restype = i32
    L.rt_render_opts_default.argtypes = [vp]
    L.rt_render_opts_default.restype = None
    sigs = {
        "rt_context_create": [i32, vp],
        "rt_context_destroy": [vp],
        "rt_context_set_stream": [vp, vp],
        "rt_context_synchronize": [vp],
        "rt_scene_create": [vp, vp, vp],
        "rt_scene_destroy": [vp],
        "rt_scene_set_area_light": [vp, vp],
        "rt_render": [vp, vp, vp, vp, vp, vp, vp, vp],
        "rt_render_device": [vp, vp, vp, vp, vp, vp, vp],
        "rt_render_batch": [vp, vp, vp, i32, vp, vp, vp, vp],
        "rt_gbuffer": [vp, vp, vp, vp, i32, vp],
        "rt_gbuffer_device": [vp, vp, vp, i32, vp, i32, vp],
        "rt_render_multi": [vp, vp, i32, vp, vp, vp, vp, vp, vp],
        "rt_stats_read": [vp, vp],
        "rt_stats_reset": [vp],
        "rt_trace_rays": [vp, vp, vp, vp, ctypes.c_size_t, vp, vp],
        "rt_intersect_rays": [vp, vp, vp, ctypes.c_size_t, vp],
        "rt_occluded_rays": [vp, vp, vp, vp, vp, ctypes.c_size_t, vp],
        "rt_occluded_rays_device": [vp, vp, vp, vp, vp, ctypes.c_size_t, vp],
        "rt_transmittance_rays": [vp, vp, vp, vp, vp, ctypes.c_size_t, vp],
        "rt_transmittance_rays_device": [vp, vp, vp, vp, vp, ctypes.c_size_t, vp],
        "rt_light_transmittance": [vp, vp, vp, vp, ctypes.c_size_t, vp],
        "rt_light_transmittance_device": [vp, vp, vp, vp, ctypes.c_size_t, vp],
        "rt_direct_light": [vp, vp, vp, vp, vp, ctypes.c_size_t, ctypes.c_size_t, i32, vp],
        "rt_direct_light_device": [vp, vp, vp, vp, vp, ctypes.c_size_t, ctypes.c_size_t, i32, vp],
        "rt_direct_light_rays": [vp, vp, vp, vp, ctypes.c_size_t, i32, vp],
        "rt_direct_light_rays_device": [vp, vp, vp, vp, ctypes.c_size_t, i32, vp],
        "rt_scatter_rays": [vp, vp, vp, vp, ctypes.c_size_t, i32, vp],
        "rt_scatter_rays_device": [vp, vp, vp, vp, ctypes.c_size_t, i32, vp],
        "rt_camera_rays": [vp, vp, vp, i32, vp],
        "rt_camera_rays_device": [vp, vp, vp, i32, vp],
        "rt_closest_rays": [vp, vp, vp, vp, ctypes.c_size_t, i32, vp],
        "rt_closest_rays_device": [vp, vp, vp, vp, ctypes.c_size_t, i32, vp],
        "rt_trace_rays_device": [vp, vp, vp, vp, ctypes.c_size_t, vp],
        "rt_accumulate_samples": [vp, vp, vp, vp, i32, i32, vp],
        "rt_accumulate_samples_device": [vp, vp, vp, vp, i32, i32, vp],
        "rt_resolve": [vp, vp, ctypes.c_size_t, i32, i32, vp, vp, vp],
        "rt_resolve_device": [vp, vp, ctypes.c_size_t, i32, i32, vp, vp, vp],
        "rt_accumulate_adaptive": [vp, vp, vp, vp, vp, i32, i32, vp, vp, vp],
        "rt_accumulate_adaptive_device": [vp, vp, vp, vp, vp, i32, i32, vp, vp, vp],
        "rt_resolve_counts": [vp, vp, vp, ctypes.c_size_t, i32, vp, vp, vp],
        "rt_resolve_counts_device": [vp, vp, vp, ctypes.c_size_t, i32, vp, vp, vp],
        "rt_debug_adaptive_listed": [vp, vp],
        "rt_tonemap": [vp, vp, ctypes.c_size_t, i32, vp],
        "rt_debug_f64_ops": [vp, vp, vp, ctypes.c_size_t, vp],
        "rt_debug_vec_ops": [vp, vp, ctypes.c_size_t, vp],
        "rt_comm_unique_id": [vp],
        "rt_comm_create": [vp, i32, i32, vp, vp],
        "rt_comm_create_ex": [vp, i32, i32, vp, ctypes.c_long, vp],
        "rt_comm_set_timeout": [vp, ctypes.c_long],
        "rt_comm_create_all": [vp, i32, vp],
        "rt_comm_create_local": [vp, i32, vp],
        "rt_comm_destroy": [vp],
        "rt_comm_info": [vp, vp, vp],
        "rt_comm_set_root_weight": [vp, i32],
        "rt_render_gather": [vp, vp, vp, vp, i32, vp, vp, vp],
        "rt_render_gather_all": [vp, vp, i32, vp, vp, i32, vp, vp, vp],
        "rt_render_gather_batch": [vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp],
        "rt_render_gather_all_batch": [vp, vp, i32, vp, i32, vp, i32, vp, vp, vp],
        "rt_comm_timing": [vp, vp, i32],
        "rt_comm_synchronize": [vp],
        "rt_queue_create": [vp, i32, vp],
        "rt_queue_destroy": [vp],
        "rt_queue_submit": [vp, vp, vp, vp, vp, vp, vp, vp],
        "rt_queue_wait": [vp, ctypes.c_uint64],
        "rt_queue_synchronize": [vp],
        "rt_debug_tile_order": [vp, vp, vp, vp, vp, ctypes.c_size_t, vp, vp, vp],
        "rt_debug_cone_table": [vp, vp, vp],
        "rt_debug_shadow_table": [vp, vp, vp],
        "rt_debug_tile_class": [vp, vp, vp],
        "rt_debug_plane_clear": [vp, vp, vp],
        "rt_debug_tile_split": [vp, vp, vp],
        "rt_debug_tile_shadowed": [vp, vp, vp],
        "rt_debug_fixup_count": [vp, vp],
        "rt_debug_assemble_rows": [vp, vp, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32,
                                   ctypes.c_uint32, ctypes.c_uint32, vp],
    }
    # a _keyed entry takes its sibling's arguments, then the rt_area_keys record
    for query in ("rt_light_transmittance", "rt_direct_light", "rt_direct_light_rays",
                  "rt_scatter_rays"):
        for form in ("", "_device"):
            sigs[query + "_keyed" + form] = sigs[query + form] + [vp]
    for name, args in sigs.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            if "RTAMD_LIB" in os.environ:  # an older A/B build (tools/variants): dev use only
                continue
            raise
        fn.argtypes = args
        fn.restype = i32
    _lib = L
    return L


def build_info() -> dict:
    """The loaded library's build record (rt_build_info), plus `matches_tree`: whether its
    source_sha256 equals the digest of the sources in this tree (raytracingengine_amd/build.py
    source_digest) — False means the binary is stale against its sources."""
    import json
    info = json.loads(load_library().rt_build_info().decode())
    from . import build
    info["matches_tree"] = info.get("source_sha256") == build.source_digest()
    return info


def _check(status: int):
    if status != RT_OK:
        raise RtError(status, _lib.rt_last_error().decode(errors="replace"))


def rendered_rows(o: RenderOpts, height: int) -> int:
    """Rows a render call produces (rt_capi.h rt_render_opts: a row range, or block-cyclic row
    blocks when row_cycle > 1) — the height of the output buffers."""
    r1 = min(o.row_end, height) if o.row_end else height
    if r1 <= o.row_begin:
        return 0
    if o.row_cycle <= 1 or o.row_block == 0:
        return r1 - o.row_begin
    stride = o.row_block * o.row_cycle
    return sum(min(o.row_block, r1 - b) for b in range(o.row_begin, r1, stride))


def default_opts(**kw) -> RenderOpts:
    o = RenderOpts()
    load_library().rt_render_opts_default(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _query_opts(bias=None, no_bvh: bool = False, max_recursion=None, seed=None) -> RenderOpts:
    """The options of a batch query: the defaults, RT_FLAG_NO_BVH alone in the flags, and the
    bias, max_recursion and seed where the query takes them."""
    o = default_opts(flags=RT_FLAG_NO_BVH if no_bvh else 0)
    if seed is not None:
        o.seed = seed
    if bias is not None:
        o.bias = bias
    if max_recursion is not None:
        o.max_recursion = max_recursion
    return o


def device_count() -> int:
    return load_library().rt_device_count()


class AdaptiveRule(ctypes.Structure):
    """rt_adaptive_rule (rt_capi.h): the stop rule of the adaptive entries."""
    _fields_ = [("tolerance", ctypes.c_double), ("lum_floor", ctypes.c_double),
                ("min_samples", ctypes.c_int32), ("_pad0", ctypes.c_int32)]


# The defaults of DeviceScene.accumulate_adaptive[_device] and render_adaptive.
ADAPTIVE_TOLERANCE = 0.05   # render_adaptive's: a row of profiles/adaptive_time.txt (README)
ADAPTIVE_MIN_SAMPLES = 4
ADAPTIVE_LUM_FLOOR = 0.01


class AdaptiveState(NamedTuple):
    """The state of an adaptive frame, one row per pixel of the row set: sum float64 [n,3],
    moments float64 [n,2] {m1, m2}, count int32 [n] — torch tensors from the _device entry, numpy
    arrays from the host entry."""
    sum: object
    moments: object
    count: object


def progressive_schedule(aa_samples: int) -> list:
    """The default steps of DeviceScene.render_progressive: the sample counts 1, 2, 4, ... below
    max(1, aa_samples), then that count itself.  A pure function."""
    n = max(1, int(aa_samples))
    steps, k = [], 1
    while k < n:
        steps.append(k)
        k *= 2
    return steps + [n]


class Context:
    """One HIP device + stream (rt_context)."""

    def __init__(self, device: int = 0):
        L = load_library()
        self._h = ctypes.c_void_p()
        _check(L.rt_context_create(device, ctypes.byref(self._h)))
        self.device = device

    def close(self):
        if self._h:
            _lib.rt_context_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._h

    def set_stream(self, stream_ptr: int | None):
        _check(_lib.rt_context_set_stream(self._h, stream_ptr))

    def synchronize(self):
        _check(_lib.rt_context_synchronize(self._h))

    def scene(self, sc: SceneData) -> "DeviceScene":
        return DeviceScene(self, sc)

    def stats(self) -> Stats:
        s = Stats()
        _check(_lib.rt_stats_read(self._h, ctypes.byref(s)))
        return s

    def reset_stats(self):
        _check(_lib.rt_stats_reset(self._h))

    def tonemap(self, hdr: np.ndarray, op: int) -> np.ndarray:
        hdr = np.ascontiguousarray(hdr, np.float64).reshape(-1, 3)
        planes = 7 if op == TONEMAP_ALL else 1
        out = np.empty((planes, hdr.shape[0], 3), np.uint8)
        _check(_lib.rt_tonemap(self._h, hdr.ctypes.data, hdr.shape[0], op, out.ctypes.data))
        return out if planes > 1 else out[0]

    def debug_f64_ops(self, x: np.ndarray, y: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float64)
        y = np.ascontiguousarray(y, np.float64)
        out = np.empty((x.size, 5), np.float64)
        _check(_lib.rt_debug_f64_ops(self._h, x.ctypes.data, y.ctypes.data, x.size,
                                     out.ctypes.data))
        return out

    def debug_assemble_rows(self, gathered: np.ndarray, height: int, block: int, n: int,
                            max_rows: int) -> np.ndarray:
        """rank 0's assembly step alone: gathered uint8 [n, max_rows, row_bytes] -> image rows."""
        g = np.ascontiguousarray(gathered, np.uint8).reshape(n, max_rows, -1)
        out = np.empty((height, g.shape[2]), np.uint8)
        _check(_lib.rt_debug_assemble_rows(self._h, g.ctypes.data, g.shape[2], height, block, n,
                                           max_rows, out.ctypes.data))
        return out

    def _debug_counter(self, entry) -> tuple[int, int]:
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        _check(entry(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def debug_cone_table(self) -> tuple[int, int]:
        """Packet-kernel frames enqueued so far (with, without) a camera-cone table."""
        return self._debug_counter(_lib.rt_debug_cone_table)

    def debug_shadow_table(self) -> tuple[int, int]:
        """Packet-kernel frames enqueued so far (with, without) a shadow-cull table."""
        return self._debug_counter(_lib.rt_debug_shadow_table)

    def debug_tile_class(self) -> tuple[int, int]:
        """Packet-kernel frames enqueued so far (with, without) tile class words."""
        return self._debug_counter(_lib.rt_debug_tile_class)

    def debug_plane_clear(self) -> tuple[int, int]:
        """Packet-kernel frames enqueued so far (with, without) shadow-plane keep masks."""
        return self._debug_counter(_lib.rt_debug_plane_clear)

    def debug_tile_split(self) -> tuple[int, int]:
        """Fix-up variant frames enqueued so far (as a split launch, as a single launch)."""
        return self._debug_counter(_lib.rt_debug_tile_split)

    def debug_tile_shadowed(self) -> tuple[int, int]:
        """Fix-up variant frames enqueued so far (with, without) a launch over shadowed tiles."""
        return self._debug_counter(_lib.rt_debug_tile_shadowed)

    def debug_fixup_count(self) -> int:
        """Pixels the last fix-up variant launch of this context queued for its fix-up launch."""
        n = ctypes.c_uint32()
        _check(_lib.rt_debug_fixup_count(self._h, ctypes.byref(n)))
        return n.value

    def debug_adaptive_listed(self) -> int:
        """Pixels the latest adaptive call of this context listed for its list kernel."""
        n = ctypes.c_uint32()
        _check(_lib.rt_debug_adaptive_listed(self._h, ctypes.byref(n)))
        return n.value

    def debug_vec_ops(self, v: np.ndarray) -> np.ndarray:
        v = np.ascontiguousarray(v, np.float64).reshape(-1, 3)
        out = np.empty((v.shape[0], 16), np.float64)
        _check(_lib.rt_debug_vec_ops(self._h, v.ctypes.data, v.shape[0], out.ctypes.data))
        return out


class DeviceScene:
    """A scene uploaded to HBM (rt_scene) plus the camera it is rendered with."""

    def __init__(self, ctx: Context, sc: SceneData):
        self.ctx = ctx
        self.data = sc
        self._arrays = (sc.sphere_array(), sc.plane_array(), sc.triangle_array(), sc.light_array())
        sp, pl, tr, lt = self._arrays
        desc = SceneDesc(sp.ctypes.data if len(sp) else None, len(sp),
                         pl.ctypes.data if len(pl) else None, len(pl),
                         tr.ctypes.data if len(tr) else None, len(tr),
                         lt.ctypes.data if len(lt) else None, len(lt))
        self._h = ctypes.c_void_p()
        _check(_lib.rt_scene_create(ctx.handle, ctypes.byref(desc), ctypes.byref(self._h)))
        self.camera = sc.camera.to_struct()
        self._area = None
        if sc.area_light is not None:
            self._area = sc.area_light.to_struct()
            _check(_lib.rt_scene_set_area_light(self._h, self._area.ctypes.data))

    def close(self):
        if self._h:
            _lib.rt_scene_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def render(self, *, hdr64=True, hdr32=False, tonemap: int = TONEMAP_NONE, opts=None,
               stats=False, **opt_kw):
        """Synchronous render into host arrays (rt_render).  Returns dict of outputs."""
        cam = self.data.camera
        o = opts if opts is not None else default_opts(tonemap=tonemap, **opt_kw)
        if opts is None:
            o.tonemap = tonemap
        rows = rendered_rows(o, cam.height)
        out = {}
        a64 = np.empty((rows, cam.width, 3), np.float64) if hdr64 else None
        a32 = np.empty((rows, cam.width, 3), np.float32) if hdr32 else None
        ldr = np.empty((rows, cam.width, 3), np.uint8) if tonemap != TONEMAP_NONE else None
        st = Stats()
        _check(_lib.rt_render(self.ctx.handle, self._h, self.camera.ctypes.data, ctypes.byref(o),
                              a64.ctypes.data if a64 is not None else None,
                              a32.ctypes.data if a32 is not None else None,
                              ldr.ctypes.data if ldr is not None else None,
                              ctypes.byref(st) if stats else None))
        if a64 is not None:
            out["hdr64"] = a64
        if a32 is not None:
            out["hdr32"] = a32
        if ldr is not None:
            out["ldr"] = ldr
        if stats:
            out["trace_rays"] = st.trace_rays
            out["shadow_rays"] = st.shadow_rays
        return out

    def render_host(self, h_hdr64: int | None, h_hdr32: int | None, h_ldr: int | None,
                    opts: RenderOpts, stats: bool = False):
        """Synchronous render into caller-owned HOST buffers (rt_render): the drop-in
        RenderImage() path, device-to-host copies included."""
        st = Stats()
        _check(_lib.rt_render(self.ctx.handle, self._h, self.camera.ctypes.data, ctypes.byref(opts),
                              h_hdr64, h_hdr32, h_ldr, ctypes.byref(st) if stats else None))
        return st if stats else None

    def trace_rays(self, rays: np.ndarray, stats=False, **opt_kw):
        """Batch TraceRay at depth 0 (rt_trace_rays): rays [n,6] -> rgb [n,3]."""
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
        out = np.empty((rays.shape[0], 3), np.float64)
        o = default_opts(**opt_kw)
        st = Stats()
        _check(_lib.rt_trace_rays(self.ctx.handle, self._h, ctypes.byref(o), rays.ctypes.data,
                                  rays.shape[0], out.ctypes.data,
                                  ctypes.byref(st) if stats else None))
        return (out, st) if stats else out

    def intersect_rays(self, rays: np.ndarray) -> np.ndarray:
        """Batch IntersectClosest (rt_intersect_rays): rays [n,6] -> hits [n,9]."""
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
        out = np.empty((rays.shape[0], 9), np.float64)
        _check(_lib.rt_intersect_rays(self.ctx.handle, self._h, rays.ctypes.data, rays.shape[0],
                                      out.ctypes.data))
        return out

    def _device(self):
        """The torch device of the context: where the tensors of the *_device methods live."""
        import torch
        return torch.device(f"cuda:{self.ctx.device}")

    def occluded(self, rays: np.ndarray, max_dist, no_bvh: bool = False) -> np.ndarray:
        """Batch IntersectAnyBefore (rt_occluded_rays): rays [n,6] and max_dist (a scalar, or
        one distance per ray) -> bool [n], True where a primitive lies at 0 < t < max_dist."""
        rays, n = _host_rows(rays, 6)
        dist = np.ascontiguousarray(np.broadcast_to(np.asarray(max_dist, np.float64), (n,)))
        out = np.empty(n, np.uint8)
        o = _query_opts(no_bvh=no_bvh)
        _check(_lib.rt_occluded_rays(self.ctx.handle, self._h, ctypes.byref(o), rays.ctypes.data,
                                     dist.ctypes.data, n, out.ctypes.data))
        return out.view(np.bool_)

    def occluded_device(self, rays, max_dist, out=None, no_bvh: bool = False):
        """Asynchronous IntersectAnyBefore on torch device tensors (rt_occluded_rays_device), on
        the context's stream: rays float64 [n,6] and max_dist float64 [n] (or a scalar, expanded
        on the device), contiguous, on this context's device.  Returns `out`, a uint8 [n] tensor
        of 0 / 1 (made when None); it is written when the context's stream reaches the launch."""
        import torch
        dev = self._device()
        n = _checked_input(rays, dev, torch.float64, 6, "rays")
        max_dist = _max_dist_tensor(max_dist, n, dev)
        out = _out_tensor(out, dev, torch.uint8, (n,))
        o = _query_opts(no_bvh=no_bvh)
        _check(_lib.rt_occluded_rays_device(self.ctx.handle, self._h, ctypes.byref(o),
                                            rays.data_ptr() if n else None,
                                            max_dist.data_ptr() if n else None, n,
                                            out.data_ptr() if n else None))
        return out

    def transmittance(self, rays: np.ndarray, max_dist, bias: float = 1e-3,
                      no_bvh: bool = False) -> np.ndarray:
        """Batch computeTransmittance (rt_transmittance_rays): rays [n,6] and max_dist (a scalar,
        or one distance per ray) -> float64 [n], the transmittance in [0,1] up to max_dist."""
        rays, n = _host_rows(rays, 6)
        dist = np.ascontiguousarray(np.broadcast_to(np.asarray(max_dist, np.float64), (n,)))
        out = np.empty(n, np.float64)
        o = _query_opts(bias, no_bvh)
        _check(_lib.rt_transmittance_rays(self.ctx.handle, self._h, ctypes.byref(o),
                                          rays.ctypes.data, dist.ctypes.data, n, out.ctypes.data))
        return out

    def transmittance_device(self, rays, max_dist, out=None, bias: float = 1e-3,
                             no_bvh: bool = False):
        """Asynchronous computeTransmittance on torch device tensors
        (rt_transmittance_rays_device), on the context's stream: rays float64 [n,6] and max_dist
        float64 [n] (or a scalar, expanded on the device), contiguous, on this context's device.
        Returns `out`, a float64 [n] tensor (made when None); it is written when the context's
        stream reaches the launch."""
        import torch
        dev = self._device()
        n = _checked_input(rays, dev, torch.float64, 6, "rays")
        max_dist = _max_dist_tensor(max_dist, n, dev)
        out = _out_tensor(out, dev, torch.float64, (n,))
        o = _query_opts(bias, no_bvh)
        _check(_lib.rt_transmittance_rays_device(self.ctx.handle, self._h, ctypes.byref(o),
                                                 rays.data_ptr() if n else None,
                                                 max_dist.data_ptr() if n else None, n,
                                                 out.data_ptr() if n else None))
        return out

    def _light_columns(self, area_keys) -> int:
        """Columns of the light-transmittance table: the point lights, and with keys the attached
        area light's samples after them."""
        keyed = area_keys is not None and self._area is not None
        return len(self._arrays[3]) + (int(self._area["samples"][0]) if keyed else 0)

    def light_transmittance(self, points: np.ndarray, bias: float = 1e-3,
                            no_bvh: bool = False, area_keys=None, seed=None) -> np.ndarray:
        """directLightning's shadow rays (rt_light_transmittance): points [n,6] {p, normal}, the
        normal facing the viewer -> float64 [n, n_lights], the transmittance from each point to
        each point light (0.0 where the reference skips the light).  area_keys (an AreaKeys; the
        draws under `seed`): rt_light_transmittance_keyed, [n, n_lights + samples] with the area
        light's samples after the lights."""
        points, n = _host_rows(points, 6)
        out = np.empty((n, self._light_columns(area_keys)), np.float64)
        o = _query_opts(bias, no_bvh, seed=seed)
        args = (self.ctx.handle, self._h, ctypes.byref(o), points.ctypes.data if n else None, n,
                out.ctypes.data if out.size else None)
        _call_level("rt_light_transmittance", args, area_keys, n)
        return out

    def light_transmittance_device(self, points, out=None, bias: float = 1e-3,
                                   no_bvh: bool = False, area_keys=None, seed=None):
        """Asynchronous rt_light_transmittance_device on the context's stream: points a
        contiguous float64 [n,6] tensor on this context's device.  Returns `out`, a float64
        [n, n_lights] tensor (made when None; a given one needs at least n*n_lights elements).
        area_keys: rt_light_transmittance_keyed_device, n_lights + samples columns."""
        import torch
        dev = self._device()
        n = _checked_input(points, dev, torch.float64, 6, "points")
        nl = self._light_columns(area_keys)
        out = _out_tensor(out, dev, torch.float64, (n, nl), need="n*columns")
        o = _query_opts(bias, no_bvh, seed=seed)
        args = (self.ctx.handle, self._h, ctypes.byref(o), points.data_ptr() if n else None, n,
                out.data_ptr() if n * nl else None)
        _call_level("rt_light_transmittance", args, area_keys, n, dev)
        return out

    def direct_light(self, points: np.ndarray, materials, outputs: int = DL_RADIANCE,
                     bias: float = 1e-3, no_bvh: bool = False, area_keys=None, seed=None) -> dict:
        """Batch directLightning (rt_direct_light): points [n,9] {p, normal facing the viewer,
        view}; materials a scene.Material or seven values (shared by all points) or an [n,7]
        array -> {"radiance" | "diffuse" | "specular": float64 [n,3]} for the DL_* bits of
        `outputs`.  area_keys (an AreaKeys; the draws under `seed`): rt_direct_light_keyed, the
        area light's samples after the point lights."""
        points, n = _host_rows(points, 9)
        m = material_rows(materials, n)
        res, ptrs = _outputs("DL", outputs, n)
        o = _query_opts(bias, no_bvh, seed=seed)
        args = (self.ctx.handle, self._h, ctypes.byref(o), points.ctypes.data if n else None,
                m.ctypes.data, m.shape[0], n, outputs, ctypes.byref(ptrs))
        _call_level("rt_direct_light", args, area_keys, n)
        return res

    def direct_light_rays(self, rays: np.ndarray, outputs: int = DL_RADIANCE, bias: float = 1e-3,
                          no_bvh: bool = False, area_keys=None, seed=None) -> dict:
        """directLightning at the first hit of every ray (rt_direct_light_rays), with the hit
        primitive's material: rays [n,6] -> the dict of direct_light; zeros where a ray misses.
        area_keys: rt_direct_light_rays_keyed."""
        rays, n = _host_rows(rays, 6)
        res, ptrs = _outputs("DL", outputs, n)
        o = _query_opts(bias, no_bvh, seed=seed)
        args = (self.ctx.handle, self._h, ctypes.byref(o), rays.ctypes.data if n else None, n,
                outputs, ctypes.byref(ptrs))
        _call_level("rt_direct_light_rays", args, area_keys, n)
        return res

    def direct_light_device(self, points, materials, outputs: int = DL_RADIANCE, out=None,
                            bias: float = 1e-3, no_bvh: bool = False, area_keys=None,
                            seed=None) -> dict:
        """Asynchronous rt_direct_light_device on the context's stream: points a contiguous
        float64 [n,9] tensor on this context's device; materials a contiguous float64 [n,7]
        tensor there, or a scene.Material / seven values on the host (shared by all points, passed
        in the kernel arguments).  Returns a dict of float64 [n,3] tensors; `out` may hold a
        tensor per requested name to write into.  area_keys: rt_direct_light_keyed_device."""
        import torch
        dev = self._device()
        n = _checked_input(points, dev, torch.float64, 9, "points")
        if torch.is_tensor(materials) and materials.numel() != 7:
            if _checked_input(materials, dev, torch.float64, 7, "materials") != n:
                raise ValueError("materials: a contiguous float64 [n,7] tensor on the device")
            m_ptr, n_m = materials.data_ptr(), n
        else:   # one material: a host record, read by the call before it returns
            if torch.is_tensor(materials):
                materials = materials.detach().cpu().numpy().reshape(7)
            host = material_rows(materials, 1)
            m_ptr, n_m = host.ctypes.data, 1
        res, ptrs = _outputs("DL", outputs, n, dev, out)
        o = _query_opts(bias, no_bvh, seed=seed)
        args = (self.ctx.handle, self._h, ctypes.byref(o), points.data_ptr() if n else None,
                m_ptr, n_m, n, outputs, ctypes.byref(ptrs))
        _call_level("rt_direct_light", args, area_keys, n, dev)
        return res

    def direct_light_rays_device(self, rays, outputs: int = DL_RADIANCE, out=None,
                                 bias: float = 1e-3, no_bvh: bool = False, area_keys=None,
                                 seed=None) -> dict:
        """Asynchronous rt_direct_light_rays_device on the context's stream: rays a contiguous
        float64 [n,6] tensor on this context's device.  Returns a dict of float64 [n,3] tensors;
        `out` may hold a tensor per requested name to write into.  area_keys:
        rt_direct_light_rays_keyed_device."""
        import torch
        dev = self._device()
        n = _checked_input(rays, dev, torch.float64, 6, "rays")
        res, ptrs = _outputs("DL", outputs, n, dev, out)
        o = _query_opts(bias, no_bvh, seed=seed)
        args = (self.ctx.handle, self._h, ctypes.byref(o), rays.data_ptr() if n else None, n,
                outputs, ctypes.byref(ptrs))
        _call_level("rt_direct_light_rays", args, area_keys, n, dev)
        return res

    def scatter(self, rays: np.ndarray, outputs: int = SC_ALL, bias: float = 1e-3,
                terminal: bool = False, no_bvh: bool = False, area_keys=None, seed=None) -> dict:
        """One TraceRay level per ray, before its children are traced (rt_scatter_rays): rays
        [n,6] -> {"value" [n,3], "refract_rays" [n,6], "reflect_rays" [n,6], "weights" [n,2] {fw,
        rw}: float64; "flags" [n] uint8: bit 0 hit, bit 1 refraction ray, bit 2 reflection ray}
        for the SC_* bits of `outputs`.  An absent child is zeros.  terminal: every ray is at the
        recursion limit (max_recursion = 0): sky, no intersection, no children.  area_keys (an
        AreaKeys; the draws under `seed`): rt_scatter_rays_keyed, the value with the area light."""
        rays, n = _host_rows(rays, 6)
        res, ptrs = _outputs("SC", outputs, n)
        o = _query_opts(bias, no_bvh, 0 if terminal else 1, seed=seed)
        args = (self.ctx.handle, self._h, ctypes.byref(o), rays.ctypes.data if n else None, n,
                outputs, ctypes.byref(ptrs))
        _call_level("rt_scatter_rays", args, area_keys, n)
        return res

    def scatter_device(self, rays, outputs: int = SC_ALL, out=None, bias: float = 1e-3,
                       terminal: bool = False, no_bvh: bool = False, area_keys=None,
                       seed=None) -> dict:
        """Asynchronous rt_scatter_rays_device on the context's stream: rays a contiguous float64
        [n,6] tensor on this context's device.  Returns the dict of scatter() as torch tensors;
        `out` may hold a tensor per requested name to write into.  area_keys:
        rt_scatter_rays_keyed_device."""
        import torch
        dev = self._device()
        n = _checked_input(rays, dev, torch.float64, 6, "rays")
        res, ptrs = _outputs("SC", outputs, n, dev, out)
        o = _query_opts(bias, no_bvh, 0 if terminal else 1, seed=seed)
        args = (self.ctx.handle, self._h, ctypes.byref(o), rays.data_ptr() if n else None, n,
                outputs, ctypes.byref(ptrs))
        _call_level("rt_scatter_rays", args, area_keys, n, dev)
        return res

    def _camera_record(self, cam):
        """(the rt_camera record, width, height) of `cam`, or of the scene's camera for None."""
        rec = self.camera if cam is None else np.ascontiguousarray(cam).reshape(-1)[:1]
        return rec, int(rec["width"][0]), int(rec["height"][0])

    def camera_rays(self, sample: int = 0, cam=None, **opts) -> np.ndarray:
        """The camera rays of AA sample `sample` (rt_camera_rays): Camera::getRay for every pixel
        of the row set of opts (seed, row_begin, row_end, row_block, row_cycle), float64
        [rows*W, 6] {o, d}, rows-local like render's pixels.  cam: an rt_camera record as
        `cameras()` makes; None: the scene's camera.  Sample 0 is never jittered."""
        rec, w, h = self._camera_record(cam)
        o = default_opts(**opts)
        out = np.empty((rendered_rows(o, h) * w, 6), np.float64)
        _check(_lib.rt_camera_rays(self.ctx.handle, rec.ctypes.data, ctypes.byref(o), sample,
                                   out.ctypes.data or 8))
        return out

    def camera_rays_device(self, sample: int = 0, cam=None, out=None, **opts):
        """Asynchronous rt_camera_rays_device on the context's stream: the rays of camera_rays()
        as a float64 [rows*W, 6] torch tensor on the context's device (`out`: a contiguous float64
        tensor of at least rows*W*6 elements to write into, returned as it is)."""
        import torch
        rec, w, h = self._camera_record(cam)
        o = default_opts(**opts)
        out = _out_tensor(out, self._device(), torch.float64, (rendered_rows(o, h) * w, 6),
                          need="rows*W*6")
        _check(_lib.rt_camera_rays_device(self.ctx.handle, rec.ctypes.data, ctypes.byref(o),
                                          sample, out.data_ptr() or 8))
        return out

    def closest(self, rays: np.ndarray, outputs: int = CH_ALL, no_bvh: bool = False) -> dict:
        """Batch IntersectClosest with selectable outputs (rt_closest_rays): rays [n,6] ->
        {"t" [n] float64, "prim" [n,2] int32 {type, index}, "normal" [n,3], "point" [n,3],
        "material" [n,7] float64} for the CH_* bits of `outputs`.  A miss: t = +inf, prim =
        {0, -1}, zeros elsewhere."""
        rays, n = _host_rows(rays, 6)
        res, ptrs = _outputs("CH", outputs, n)
        o = _query_opts(no_bvh=no_bvh)
        _check(_lib.rt_closest_rays(self.ctx.handle, self._h, ctypes.byref(o),
                                    rays.ctypes.data if n else None, n, outputs,
                                    ctypes.byref(ptrs)))
        return res

    def closest_device(self, rays, outputs: int = CH_ALL, out=None, no_bvh: bool = False) -> dict:
        """Asynchronous rt_closest_rays_device on the context's stream: rays a contiguous float64
        [n,6] tensor on this context's device.  Returns the dict of closest() as torch tensors;
        `out` may hold a tensor per requested name to write into."""
        import torch
        dev = self._device()
        n = _checked_input(rays, dev, torch.float64, 6, "rays")
        res, ptrs = _outputs("CH", outputs, n, dev, out)
        o = _query_opts(no_bvh=no_bvh)
        _check(_lib.rt_closest_rays_device(self.ctx.handle, self._h, ctypes.byref(o),
                                           rays.data_ptr() if n else None, n, outputs,
                                           ctypes.byref(ptrs)))
        return res

    def trace_rays_device(self, rays, out=None, **opts):
        """Asynchronous rt_trace_rays_device on the context's stream: TraceRay at depth 0 for a
        contiguous float64 [n,6] tensor on this context's device -> float64 [n,3] (`out`: a
        contiguous float64 tensor of at least n*3 elements to write into, returned as it is).
        opts as trace_rays (max_recursion, bias, seed, flags)."""
        import torch
        dev = self._device()
        n = _checked_input(rays, dev, torch.float64, 6, "rays")
        out = _out_tensor(out, dev, torch.float64, (n, 3), need="n*3")
        o = default_opts(**opts)
        _check(_lib.rt_trace_rays_device(self.ctx.handle, self._h, ctypes.byref(o),
                                         rays.data_ptr() if n else None, n,
                                         out.data_ptr() if n else None))
        return out

    def accumulate(self, sample_begin: int, sample_end: int, sum=None, cam=None,
                   **opts) -> np.ndarray:
        """Add the AA samples [sample_begin, sample_end) of every pixel of the row set of opts to
        a host sum (rt_accumulate_samples): float64 [rows*W, 3], GeneratePixelAt's loop in its
        order.  sum: the sum so far, required when sample_begin > 0 (a contiguous float64 array of
        rows*W*3 elements is updated in place and returned); with sample_begin == 0 its contents
        are not read.  cam as camera_rays; opts: max_recursion, bias, seed, the row set, flags."""
        rec, w, h = self._camera_record(cam)
        o = default_opts(**opts)
        n = rendered_rows(o, h) * w
        if sum is None:
            if sample_begin > 0:
                raise ValueError("sum: required when sample_begin > 0")
            sum = np.empty((n, 3), np.float64)
        elif not (isinstance(sum, np.ndarray) and sum.dtype == np.float64
                  and sum.flags.c_contiguous and sum.flags.writeable and sum.size == 3 * n):
            sum = np.array(sum, np.float64).reshape(n, 3)
        _check(_lib.rt_accumulate_samples(self.ctx.handle, self._h, rec.ctypes.data,
                                          ctypes.byref(o), sample_begin, sample_end,
                                          sum.ctypes.data or 8))
        return sum.reshape(n, 3)

    def accumulate_device(self, sample_begin: int, sample_end: int, sum=None, cam=None, **opts):
        """Asynchronous rt_accumulate_samples_device on the context's stream: the sum of
        accumulate() as a float64 [rows*W, 3] torch tensor on the context's device.  sum: the
        tensor to add to (contiguous float64, at least rows*W*3 elements, returned as it is),
        required when sample_begin > 0; with sample_begin == 0 it need not be initialised."""
        import torch
        rec, w, h = self._camera_record(cam)
        o = default_opts(**opts)
        if sum is None and sample_begin > 0:
            raise ValueError("sum: required when sample_begin > 0")
        sum = _out_tensor(sum, self._device(), torch.float64, (rendered_rows(o, h) * w, 3), "sum",
                          "rows*W*3")
        _check(_lib.rt_accumulate_samples_device(self.ctx.handle, self._h, rec.ctypes.data,
                                                 ctypes.byref(o), sample_begin, sample_end,
                                                 sum.data_ptr() or 8))
        return sum

    def resolve(self, sum, samples: int, tonemap: int = TONEMAP_NONE, hdr64: bool = True,
                hdr32: bool = False) -> dict:
        """sum / samples as render's outputs (rt_resolve): {"hdr64" float64 [n,3], "hdr32" float32
        [n,3], "ldr" uint8 [n,3] — [7,n,3] for TONEMAP_ALL — when tonemap is not TONEMAP_NONE}
        from a float64 [n,3] host sum.  With samples = 1 the bytes are Context.tonemap's."""
        sum, n = _host_rows(sum, 3)
        out = {}
        if hdr64:
            out["hdr64"] = np.empty((n, 3), np.float64)
        if hdr32:
            out["hdr32"] = np.empty((n, 3), np.float32)
        if tonemap != TONEMAP_NONE:
            out["ldr"] = np.empty((7, n, 3) if tonemap == TONEMAP_ALL else (n, 3), np.uint8)
        ptr = {k: (v.ctypes.data or 8) for k, v in out.items()}
        _check(_lib.rt_resolve(self.ctx.handle, sum.ctypes.data or 8, n, samples, tonemap,
                               ptr.get("hdr64"), ptr.get("hdr32"), ptr.get("ldr")))
        return out

    def resolve_device(self, sum, samples: int, tonemap: int = TONEMAP_NONE, hdr64: bool = True,
                       hdr32: bool = False, out=None) -> dict:
        """Asynchronous rt_resolve_device on the context's stream: resolve() on a contiguous
        float64 [n,3] tensor on the context's device, the outputs torch tensors there (`out` may
        hold a tensor per requested name to write into).  No host synchronisation: after
        accumulate_device on the same context the sum is read in stream order."""
        import torch
        dev = self._device()
        n = _checked_input(sum, dev, torch.float64, 3, "sum")
        want = []
        if hdr64:
            want.append(("hdr64", torch.float64, (n, 3)))
        if hdr32:
            want.append(("hdr32", torch.float32, (n, 3)))
        if tonemap != TONEMAP_NONE:
            want.append(("ldr", torch.uint8, (7, n, 3) if tonemap == TONEMAP_ALL else (n, 3)))
        res = {name: _out_tensor(None if out is None else out.get(name), dev, tdt, shape,
                                 f"out[{name!r}]", str(math.prod(shape)))
               for name, tdt, shape in want}
        # never a NULL pointer for a requested output or the sum, an empty tensor's included
        ptr = {k: (v.data_ptr() or 8) for k, v in res.items()}
        _check(_lib.rt_resolve_device(self.ctx.handle, sum.data_ptr() or 8, n, samples, tonemap,
                                      ptr.get("hdr64"), ptr.get("hdr32"), ptr.get("ldr")))
        return res

    def render_progressive(self, schedule=None, tonemap: int = TONEMAP_NONE, hdr64: bool = True,
                           hdr32: bool = False, cam=None, **opts):
        """A generator over a frame that refines: after each step k of `schedule` (increasing
        sample counts ending at max(1, aa_samples); None: progressive_schedule) it yields
        (k, outputs), outputs = resolve_device(the sum of samples [0, k), k) as device tensors,
        enqueued on the context's stream and not synchronised.  One sum is continued from step to
        step, so the last step's outputs are the frame's, and each step's outputs are new
        tensors.  Stop iterating to stop rendering."""
        rec, _, _ = self._camera_record(cam)
        aa = max(1, int(rec["aa_samples"][0]))
        steps = progressive_schedule(aa) if schedule is None else [int(k) for k in schedule]
        if (not steps or steps[0] < 1 or steps[-1] != aa
                or any(b <= a for a, b in zip(steps, steps[1:]))):
            raise ValueError("schedule: increasing sample counts from at least 1, ending at "
                             "max(1, aa_samples)")
        acc, done = None, 0
        for k in steps:
            acc = self.accumulate_device(done, k, sum=acc, cam=cam, **opts)
            done = k
            yield k, self.resolve_device(acc, k, tonemap=tonemap, hdr64=hdr64, hdr32=hdr32)

    def accumulate_adaptive(self, sample_end: int, tolerance: float,
                            min_samples: int = ADAPTIVE_MIN_SAMPLES,
                            lum_floor: float = ADAPTIVE_LUM_FLOOR, state=None, cam=None,
                            fresh=None, **opts) -> AdaptiveState:
        """Continue every pixel of the row set of opts up to sample_end samples while the stop
        rule wants more (rt_accumulate_adaptive; the rule is in rt_capi.h): a pixel stops once it
        has min_samples samples and the squared standard error of its mean luminance is at most
        (tolerance * max(mean, lum_floor))**2.  state: the AdaptiveState to continue (its
        contiguous numpy arrays are updated in place); None starts a fresh one.  fresh=True with
        a state starts afresh in its arrays, whose contents are then not read.  cam and opts as
        accumulate."""
        rec, w, h = self._camera_record(cam)
        o = default_opts(**opts)
        n = rendered_rows(o, h) * w
        rule = AdaptiveRule(tolerance, lum_floor, min_samples, 0)
        if state is None:
            state = AdaptiveState(np.empty((n, 3), np.float64), np.empty((n, 2), np.float64),
                                  np.empty(n, np.int32))
            fresh = True
        else:
            for a, dt, k in zip(state, (np.float64, np.float64, np.int32), (3, 2, 1)):
                if not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous
                        and a.flags.writeable and a.size == k * n):
                    raise ValueError("state: contiguous writable arrays sum float64 [n,3], "
                                     "moments float64 [n,2], count int32 [n], n = rows*W")
        _check(_lib.rt_accumulate_adaptive(self.ctx.handle, self._h, rec.ctypes.data,
                                           ctypes.byref(o), ctypes.byref(rule), 1 if fresh else 0,
                                           sample_end, *(a.ctypes.data or 8 for a in state)))
        return state

    def accumulate_adaptive_device(self, sample_end: int, tolerance: float,
                                   min_samples: int = ADAPTIVE_MIN_SAMPLES,
                                   lum_floor: float = ADAPTIVE_LUM_FLOOR, state=None, cam=None,
                                   fresh=None, **opts) -> AdaptiveState:
        """Asynchronous rt_accumulate_adaptive_device on the context's stream: accumulate_adaptive
        on torch tensors on the context's device.  state None: a fresh state in new tensors;
        fresh=True with a state: a fresh one in its tensors, which need no initialisation."""
        import torch
        rec, w, h = self._camera_record(cam)
        o = default_opts(**opts)
        n = rendered_rows(o, h) * w
        rule = AdaptiveRule(tolerance, lum_floor, min_samples, 0)
        fresh = fresh or state is None
        dev = self._device()
        given = (None, None, None) if state is None else state
        state = AdaptiveState(
            _out_tensor(given[0], dev, torch.float64, (n, 3), "state.sum", "rows*W*3"),
            _out_tensor(given[1], dev, torch.float64, (n, 2), "state.moments", "rows*W*2"),
            _out_tensor(given[2], dev, torch.int32, (n,), "state.count", "rows*W"))
        _check(_lib.rt_accumulate_adaptive_device(self.ctx.handle, self._h, rec.ctypes.data,
                                                  ctypes.byref(o), ctypes.byref(rule),
                                                  1 if fresh else 0, sample_end,
                                                  *(t.data_ptr() or 8 for t in state)))
        return state

    def resolve_counts(self, sum, count, tonemap: int = TONEMAP_NONE, hdr64: bool = True,
                       hdr32: bool = False) -> dict:
        """resolve() with each pixel's own count as the divisor (rt_resolve_counts): sum float64
        [n,3], count int32 [n]; a pixel whose count is 0 is (0, 0, 0)."""
        sum, n = _host_rows(sum, 3)
        count = np.ascontiguousarray(count, np.int32).reshape(-1)
        if count.size != n:
            raise ValueError("count: one int32 per pixel of the sum")
        out = {}
        if hdr64:
            out["hdr64"] = np.empty((n, 3), np.float64)
        if hdr32:
            out["hdr32"] = np.empty((n, 3), np.float32)
        if tonemap != TONEMAP_NONE:
            out["ldr"] = np.empty((7, n, 3) if tonemap == TONEMAP_ALL else (n, 3), np.uint8)
        ptr = {k: (v.ctypes.data or 8) for k, v in out.items()}
        _check(_lib.rt_resolve_counts(self.ctx.handle, sum.ctypes.data or 8, count.ctypes.data or 8,
                                      n, tonemap, ptr.get("hdr64"), ptr.get("hdr32"),
                                      ptr.get("ldr")))
        return out

    def resolve_counts_device(self, sum, count, tonemap: int = TONEMAP_NONE, hdr64: bool = True,
                              hdr32: bool = False, out=None) -> dict:
        """Asynchronous rt_resolve_counts_device on the context's stream: resolve_counts() on a
        contiguous float64 [n,3] sum and int32 [n] count on the context's device, the outputs as
        resolve_device's."""
        import torch
        dev = self._device()
        n = _checked_input(sum, dev, torch.float64, 3, "sum")
        if _checked_input(count, dev, torch.int32, 1, "count") != n:
            raise ValueError("count: one int32 per pixel of the sum")
        want = []
        if hdr64:
            want.append(("hdr64", torch.float64, (n, 3)))
        if hdr32:
            want.append(("hdr32", torch.float32, (n, 3)))
        if tonemap != TONEMAP_NONE:
            want.append(("ldr", torch.uint8, (7, n, 3) if tonemap == TONEMAP_ALL else (n, 3)))
        res = {name: _out_tensor(None if out is None else out.get(name), dev, tdt, shape,
                                 f"out[{name!r}]", str(math.prod(shape)))
               for name, tdt, shape in want}
        ptr = {k: (v.data_ptr() or 8) for k, v in res.items()}
        _check(_lib.rt_resolve_counts_device(self.ctx.handle, sum.data_ptr() or 8,
                                             count.data_ptr() or 8, n, tonemap, ptr.get("hdr64"),
                                             ptr.get("hdr32"), ptr.get("ldr")))
        return res

    def render_adaptive(self, tolerance: float = ADAPTIVE_TOLERANCE,
                        min_samples: int = ADAPTIVE_MIN_SAMPLES,
                        lum_floor: float = ADAPTIVE_LUM_FLOOR, schedule=None,
                        tonemap: int = TONEMAP_NONE, hdr64: bool = True, hdr32: bool = False,
                        cam=None, **opts):
        """render_progressive with the stop rule: after each step k of `schedule` it yields
        (k, outputs), outputs = resolve_counts_device of one state continued to k samples, with
        outputs["samples"] the state's count tensor (int32 [n], the same tensor at every step:
        copy it to keep a step's counts).  Enqueued on the context's stream, not synchronised."""
        rec, _, _ = self._camera_record(cam)
        aa = max(1, int(rec["aa_samples"][0]))
        steps = progressive_schedule(aa) if schedule is None else [int(k) for k in schedule]
        if (not steps or steps[0] < 1 or steps[-1] != aa
                or any(b <= a for a, b in zip(steps, steps[1:]))):
            raise ValueError("schedule: increasing sample counts from at least 1, ending at "
                             "max(1, aa_samples)")
        state = None
        for k in steps:
            state = self.accumulate_adaptive_device(k, tolerance, min_samples, lum_floor,
                                                    state=state, cam=cam, **opts)
            out = self.resolve_counts_device(state.sum, state.count, tonemap=tonemap, hdr64=hdr64,
                                             hdr32=hdr32)
            out["samples"] = state.count
            yield k, out

    def debug_tile_order(self):
        """The packet kernel's tile-order state for this scene's camera (rt_debug_tile_order):
        (state, order[tiles] or None, cost[tiles, waves] or None)."""
        tiles, waves, state = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_int()
        _check(_lib.rt_debug_tile_order(self.ctx.handle, self._h, self.camera.ctypes.data, None,
                                        None, 0, ctypes.byref(tiles), ctypes.byref(waves),
                                        ctypes.byref(state)))
        if state.value == 0:
            return 0, None, None
        n, w = tiles.value, waves.value
        order = np.empty(n, np.uint32)
        cost = np.empty(n * w, np.uint32)
        _check(_lib.rt_debug_tile_order(self.ctx.handle, self._h, self.camera.ctypes.data,
                                        order.ctypes.data if state.value == 2 else None,
                                        cost.ctypes.data, cost.size, ctypes.byref(tiles),
                                        ctypes.byref(waves), ctypes.byref(state)))
        return state.value, (order if state.value == 2 else None), cost.reshape(n, w)

    def render_device(self, d_hdr64: int | None, d_hdr32: int | None, d_ldr: int | None,
                      opts: RenderOpts):
        """Asynchronous render into device pointers (rt_render_device)."""
        _check(_lib.rt_render_device(self.ctx.handle, self._h, self.camera.ctypes.data,
                                     ctypes.byref(opts), d_hdr64, d_hdr32, d_ldr))

    def cameras(self, positions) -> np.ndarray:
        """rt_camera records of this scene's camera moved to each of `positions` ([n, 3])."""
        pos = np.asarray(positions, np.float64).reshape(-1, 3)
        cams = np.repeat(self.camera, len(pos))
        cams["position"] = pos
        return cams

    def render_batch(self, cams: np.ndarray, d_hdr64: int | None, d_hdr32: int | None,
                     d_ldr: int | None, opts: RenderOpts):
        """Asynchronous render of len(cams) frames into device buffers holding them back to
        back (rt_render_batch)."""
        cams = np.ascontiguousarray(cams)
        _check(_lib.rt_render_batch(self.ctx.handle, self._h, cams.ctypes.data, len(cams),
                                    ctypes.byref(opts), d_hdr64, d_hdr32, d_ldr))

    def gbuffer(self, outputs: int = GB_ALL, cams: np.ndarray | None = None, opts=None) -> dict:
        """The frame's G-buffer as host arrays (rt_gbuffer; with `cams`, an rt_camera array as
        `cameras()` makes, one frame per camera through rt_gbuffer_device): {name: array} for the
        outputs requested (GB_* bits), shaped [frames,] rows, W[, k] — depth float64, depth_norm
        float32, normal float64 ×3, prim int32 ×2 {type, index}, albedo float32 ×3."""
        o = opts if opts is not None else default_opts()
        cam = self.data.camera
        rows = rendered_rows(o, cam.height)
        if cams is None:
            out = {n: np.empty(s, d) for n, (s, d) in
                   gbuffer_layout(outputs, cam.width, rows).items()}
            ptrs = GBufferPtrs(**{n: a.ctypes.data for n, a in out.items()})
            _check(_lib.rt_gbuffer(self.ctx.handle, self._h, self.camera.ctypes.data,
                                   ctypes.byref(o), outputs, ctypes.byref(ptrs)))
            return out
        import torch
        cams = np.ascontiguousarray(cams)
        lay = gbuffer_layout(outputs, cam.width, rows, len(cams))
        dev = {n: torch.empty(int(np.prod(s)) * d.itemsize, dtype=torch.uint8,
                              device=f"cuda:{self.ctx.device}") for n, (s, d) in lay.items()}
        self.gbuffer_device(outputs, {n: t.data_ptr() for n, t in dev.items()}, cams=cams, opts=o)
        self.ctx.synchronize()
        return {n: dev[n].cpu().numpy().view(d).reshape(s) for n, (s, d) in lay.items()}

    def gbuffer_device(self, outputs: int, ptrs: dict, cams: np.ndarray | None = None, opts=None):
        """Asynchronous G-buffer pass into raw device pointers (rt_gbuffer_device): `ptrs` maps
        output names (depth, depth_norm, normal, prim, albedo) to device addresses holding
        len(cams) frames back to back (`cams` None: this scene's camera, one frame)."""
        o = opts if opts is not None else default_opts()
        cams = self.camera if cams is None else np.ascontiguousarray(cams)
        p = GBufferPtrs(**{n: int(v) for n, v in ptrs.items() if v})
        _check(_lib.rt_gbuffer_device(self.ctx.handle, self._h, cams.ctypes.data, len(cams),
                                      ctypes.byref(o), outputs, ctypes.byref(p)))


def render_multi(scenes: list, *, hdr64=True, tonemap: int = TONEMAP_NONE, stats=False,
                 row_block: int = 0, **opt_kw) -> dict:
    """One frame over several contexts (rt_render_multi): `scenes` are DeviceScenes of the same
    SceneData, one per context; block-cyclic rows, gathered to the first context's device and
    copied to the host from there (RTAMD_MULTI_HOST=1, or no framebuffer at all: each context's
    rows copied to the host by itself).  With stats, `launches` is the rt_stats member: under
    RT_FLAG_TIME_KERNEL one per context with rows on the host path, 1 on the gathered one."""
    L = load_library()
    n = len(scenes)
    cam = scenes[0].data.camera
    o = default_opts(tonemap=tonemap, row_block=row_block, **opt_kw)
    ctxs = (ctypes.c_void_p * n)(*[ds.ctx.handle for ds in scenes])
    scs = (ctypes.c_void_p * n)(*[ds._h for ds in scenes])
    a64 = np.empty((cam.height, cam.width, 3), np.float64) if hdr64 else None
    ldr = np.empty((cam.height, cam.width, 3), np.uint8) if tonemap != TONEMAP_NONE else None
    st = Stats()
    _check(L.rt_render_multi(ctxs, scs, n, scenes[0].camera.ctypes.data, ctypes.byref(o),
                             a64.ctypes.data if a64 is not None else None, None,
                             ldr.ctypes.data if ldr is not None else None,
                             ctypes.byref(st) if stats else None))
    out = {}
    if a64 is not None:
        out["hdr64"] = a64
    if ldr is not None:
        out["ldr"] = ldr
    if stats:
        out["trace_rays"], out["shadow_rays"] = st.trace_rays, st.shadow_rays
        out["launches"] = st.launches
    return out


class _StdoutToStderr:
    """RCCL prints its version banner to stdout when a communicator is created; a bench's
    stdout carries exactly one JSON line, so the banner goes to stderr instead (fd level, C
    stdio flushed on both sides)."""

    def __enter__(self):
        import sys
        sys.stdout.flush()
        self._libc = ctypes.CDLL(None)
        self._libc.fflush(None)
        self._saved = os.dup(1)
        os.dup2(2, 1)
        return self

    def __exit__(self, *exc):
        self._libc.fflush(None)
        os.dup2(self._saved, 1)
        os.close(self._saved)


def comm_unique_id() -> bytes:
    """ncclGetUniqueId (rt_comm_unique_id): made on one rank, handed to all of them."""
    buf = (ctypes.c_uint8 * RT_COMM_ID_BYTES)()
    _check(load_library().rt_comm_unique_id(buf))
    return bytes(buf)


class Comm:
    """One rank of a row-tiled multi-GPU frame (rt_comm): render this rank's rows, one RCCL
    gather to rank 0, assembled into rank 0's device framebuffers (rt_render_gather)."""

    def __init__(self, ctx: Context, nranks: int, rank: int, uid: bytes, _handle=None,
                 timeout_ms: int | None = None):
        """timeout_ms: the deadline of the communicator's waits (rt_comm_create_ex; None = the
        library default, RTAMD_COMM_TIMEOUT_MS or 300 s; 0 = none)."""
        L = load_library()
        self.ctx = ctx
        self.nranks, self.rank = nranks, rank
        self._h = ctypes.c_void_p()
        if _handle is not None:
            self._h = _handle
            return
        if len(uid) != RT_COMM_ID_BYTES:
            raise ValueError("unique id must be RT_COMM_ID_BYTES bytes")
        idbuf = (ctypes.c_uint8 * RT_COMM_ID_BYTES).from_buffer_copy(uid)
        with _StdoutToStderr():
            if timeout_ms is None:
                st = L.rt_comm_create(ctx.handle, nranks, rank, idbuf, ctypes.byref(self._h))
            else:
                st = L.rt_comm_create_ex(ctx.handle, nranks, rank, idbuf, int(timeout_ms),
                                         ctypes.byref(self._h))
        _check(st)

    @classmethod
    def create_all(cls, ctxs: list) -> list:
        """n communicators over n distinct devices from this process (rt_comm_create_all)."""
        n = len(ctxs)
        hs = (ctypes.c_void_p * n)(*[c.handle for c in ctxs])
        out = (ctypes.c_void_p * n)()
        with _StdoutToStderr():
            st = load_library().rt_comm_create_all(hs, n, out)
        _check(st)
        return [cls(c, n, i, b"", _handle=ctypes.c_void_p(out[i])) for i, c in enumerate(ctxs)]

    @classmethod
    def create_local(cls, ctxs: list) -> list:
        """n communicators over n contexts of this process that may share a GPU
        (rt_comm_create_local: the gather as device copies); driven by render_gather_all."""
        n = len(ctxs)
        hs = (ctypes.c_void_p * n)(*[c.handle for c in ctxs])
        out = (ctypes.c_void_p * n)()
        _check(load_library().rt_comm_create_local(hs, n, out))
        return [cls(c, n, i, b"", _handle=ctypes.c_void_p(out[i])) for i, c in enumerate(ctxs)]

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            _lib.rt_comm_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def render_gather(self, dscene: "DeviceScene", opts: RenderOpts, outputs: int,
                      d_hdr64: int | None = None, d_hdr32: int | None = None,
                      d_ldr: int | None = None):
        """Collective (every rank): enqueue this rank's rows + the gather (+ rank 0's
        assembly into the d_* device framebuffers) on the context's stream."""
        _check(_lib.rt_render_gather(self._h, dscene._h, dscene.camera.ctypes.data,
                                     ctypes.byref(opts), outputs, d_hdr64, d_hdr32, d_ldr))

    def render_gather_batch(self, dscene: "DeviceScene", cams: np.ndarray, opts: RenderOpts,
                            outputs: int, d_hdr64: int | None = None, d_hdr32: int | None = None,
                            d_ldr: int | None = None, rank_hdr64: int | None = None,
                            rank_hdr32: int | None = None, rank_ldr: int | None = None):
        """Collective: len(cams) frames, this rank's rows of each in one launch, one gather of
        the whole batch per output, rank 0 assembles (rt_render_gather_batch); rank_* receive
        outputs rendered but not gathered (this rank's rows, frames max_rows rows apart)."""
        cams = np.ascontiguousarray(cams)
        _check(_lib.rt_render_gather_batch(self._h, dscene._h, cams.ctypes.data, len(cams),
                                           ctypes.byref(opts), outputs, d_hdr64, d_hdr32, d_ldr,
                                           rank_hdr64, rank_hdr32, rank_ldr))

    def synchronize(self):
        _check(_lib.rt_comm_synchronize(self._h))

    def set_timeout(self, timeout_ms: int):
        _check(_lib.rt_comm_set_timeout(self._h, int(timeout_ms)))

    def set_root_weight(self, weight: int):
        """Weighted row split (rt_comm_set_root_weight): rank 0 renders `weight` of the
        weight + n − 1 row sets, every other rank one; the same value on every rank."""
        _check(_lib.rt_comm_set_root_weight(self._h, int(weight)))

    def timing(self, reset: bool = False) -> GatherTiming:
        t = GatherTiming()
        _check(_lib.rt_comm_timing(self._h, ctypes.byref(t), int(reset)))
        return t


class Queue:
    """Serving frame queue (rt_queue): frames of one context rendered into device framebuffers
    with `depth` of them in flight on as many HIP streams."""

    def __init__(self, ctx: Context, depth: int = 2):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        _check(load_library().rt_queue_create(ctx.handle, depth, ctypes.byref(self._h)))

    def submit(self, dscene: "DeviceScene", opts: RenderOpts, d_hdr64: int | None = None,
               d_hdr32: int | None = None, d_ldr: int | None = None) -> int:
        t = ctypes.c_uint64()
        _check(_lib.rt_queue_submit(self._h, dscene._h, dscene.camera.ctypes.data,
                                    ctypes.byref(opts), d_hdr64, d_hdr32, d_ldr, ctypes.byref(t)))
        return t.value

    def wait(self, ticket: int):
        _check(_lib.rt_queue_wait(self._h, ticket))

    def synchronize(self):
        _check(_lib.rt_queue_synchronize(self._h))

    def close(self):
        if self._h:
            _lib.rt_queue_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_gather_all(comms: list, scenes: list, opts: RenderOpts, outputs: int,
                      d_hdr64: int | None = None, d_hdr32: int | None = None,
                      d_ldr: int | None = None):
    """rt_render_gather_all: every rank of a Comm.create_all group from this process."""
    n = len(comms)
    cs = (ctypes.c_void_p * n)(*[c.handle for c in comms])
    ss = (ctypes.c_void_p * n)(*[s._h for s in scenes])
    _check(load_library().rt_render_gather_all(cs, ss, n, scenes[0].camera.ctypes.data,
                                               ctypes.byref(opts), outputs, d_hdr64, d_hdr32,
                                               d_ldr))


def render_gather_all_batch(comms: list, scenes: list, cams: np.ndarray, opts: RenderOpts,
                            outputs: int, d_hdr64: int | None = None, d_hdr32: int | None = None,
                            d_ldr: int | None = None):
    """rt_render_gather_all_batch: a batch of frames over every rank of a Comm.create_all /
    create_local group from this process."""
    n = len(comms)
    cs = (ctypes.c_void_p * n)(*[c.handle for c in comms])
    ss = (ctypes.c_void_p * n)(*[s._h for s in scenes])
    cams = np.ascontiguousarray(cams)
    _check(load_library().rt_render_gather_all_batch(cs, ss, n, cams.ctypes.data, len(cams),
                                                     ctypes.byref(opts), outputs, d_hdr64,
                                                     d_hdr32, d_ldr))


def compose_trace(ds: "DeviceScene", rays: np.ndarray, depth: int, bias: float = 1e-3,
                  area_keys=None, seed=None, _level: int = 0) -> np.ndarray:
    """TraceRay(ray, 0) with maxRecursion = depth, composed level by level from scatter():
        TraceRay(ray, k) = value(ray) + TraceRay(refraction child, k + 1) * fw
                                      + TraceRay(reflection child, k + 1) * rw
    in the reference's order of the sum (Scene.h:172, 182, 193).  The children that exist are
    selected by the flags (an absent child adds nothing, not even a zero), and the level `depth`
    is asked with terminal=True: every ray there is at the recursion limit.  rays [n,6] -> [n,3].
    area_keys (an AreaKeys; the draws under `seed`): the scene's area light is served — every
    level is asked with depth = its level and the pixel keys of the rays its rays descend from
    (pixel None: ray i of the first level has key i), as TraceRay keys its draws."""
    rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
    keys = None
    if area_keys is not None:
        px = (np.arange(len(rays), dtype=np.uint64) if area_keys.pixel is None
              else np.asarray(area_keys.pixel, np.uint64).reshape(-1))
        keys = area_keys.at_depth(_level, px)
    if _level >= depth:
        return ds.scatter(rays, outputs=SC_VALUE, bias=bias, terminal=True, area_keys=keys,
                          seed=seed)["value"]
    s = ds.scatter(rays, outputs=SC_ALL, bias=bias, area_keys=keys, seed=seed)
    total = s["value"].copy()
    for key, bit, w in (("refract_rays", 2, 0), ("reflect_rays", 4, 1)):
        live = (s["flags"] & bit) != 0
        if live.any():
            child_keys = None if keys is None else keys.at_depth(_level + 1, keys.pixel[live])
            child = compose_trace(ds, s[key][live], depth, bias, child_keys, seed, _level + 1)
            total[live] = total[live] + child * s["weights"][live, w:w + 1]
    return total
