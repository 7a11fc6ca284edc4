"""The tensor checks of the Python binding's *_device methods (raytracingengine_amd/capi.py): the
module-level helpers every such method goes through, on CPU tensors — they need no context.
CPU only."""
import inspect

import numpy as np
import pytest
import torch

from raytracingengine_amd import capi

CPU = torch.device("cpu")
OTHER = torch.device("cuda:0")   # only compared with: no tensor is made there
HELPERS = {"_checked_input", "_out_tensor", "_outputs", "_max_dist_tensor"}
TABLES = {"DL": ([(n, b, np.float64, 3) for n, b in capi.DL_OUTPUTS], capi.DL_ALL),
          "SC": (capi.SC_OUTPUTS, capi.SC_ALL), "CH": (capi.CH_OUTPUTS, capi.CH_ALL)}


def test_checked_input():
    t = torch.zeros(12, dtype=torch.float64)
    assert capi._checked_input(t, CPU, torch.float64, 6, "rays") == 2
    assert capi._checked_input(t.reshape(4, 3), CPU, torch.float64, 3, "sum") == 4
    assert capi._checked_input(t[:0], CPU, torch.float64, 6, "rays") == 0
    text = "rays: a contiguous float64 tensor on the context's device"
    with pytest.raises(ValueError, match=text):           # a CPU tensor, the context elsewhere
        capi._checked_input(t, OTHER, torch.float64, 6, "rays")
    for bad in (t.float(),                                # float32
                torch.zeros(6, 4, dtype=torch.float64).t(),   # a non-contiguous view
                t[::2]):
        with pytest.raises(ValueError, match=text):
            capi._checked_input(bad, CPU, torch.float64, 6, "rays")
    for k, numel in ((6, 13), (6, 5), (9, 12), (3, 1)):   # numel not a multiple of k
        with pytest.raises(ValueError, match=rf"points: n\*{k} elements"):
            capi._checked_input(torch.zeros(numel, dtype=torch.float64), CPU, torch.float64, k,
                                "points")


def test_out_tensor():
    made = capi._out_tensor(None, CPU, torch.uint8, (5,))
    assert made.dtype == torch.uint8 and made.shape == (5,) and made.device == CPU
    made = capi._out_tensor(None, CPU, torch.float64, (4, 3), need="n*3")
    assert made.dtype == torch.float64 and made.shape == (4, 3) and made.is_contiguous()
    for given in (torch.zeros(12, dtype=torch.float64), torch.zeros((4, 3), dtype=torch.float64),
                  torch.zeros(40, dtype=torch.float64)):   # exactly enough, shaped, more
        assert capi._out_tensor(given, CPU, torch.float64, (4, 3), need="n*3") is given
    empty = torch.zeros(0, dtype=torch.float64)
    assert capi._out_tensor(empty, CPU, torch.float64, (0, 3)) is empty
    text = r"out: a contiguous float64 tensor of at least n\*3 elements on the device"
    for bad, dev in ((torch.zeros(11, dtype=torch.float64), CPU),        # one element too small
                     (torch.zeros(12, dtype=torch.float32), CPU),
                     (torch.zeros(12, dtype=torch.float64), OTHER),      # a CPU tensor
                     (torch.zeros(24, dtype=torch.float64)[::2], CPU)):  # a non-contiguous view
        with pytest.raises(ValueError, match=text):
            capi._out_tensor(bad, dev, torch.float64, (4, 3), need="n*3")
    with pytest.raises(ValueError, match=r"sum: a contiguous float64 tensor of at least rows\*W\*3"):
        capi._out_tensor(torch.zeros(2, dtype=torch.float64), CPU, torch.float64, (1, 3), "sum",
                         "rows*W*3")


def test_max_dist_tensor():
    d = torch.ones(4, dtype=torch.float64)
    assert capi._max_dist_tensor(d, 4, CPU) is d
    for bad, dev in ((d, OTHER), (d.float(), CPU), (torch.ones(8, dtype=torch.float64)[::2], CPU),
                     (torch.ones(5, dtype=torch.float64), CPU)):
        with pytest.raises(ValueError, match="max_dist: a scalar or a contiguous float64"):
            capi._max_dist_tensor(bad, 4, dev)


@pytest.mark.parametrize("kind", sorted(TABLES))
def test_outputs_of_every_mask(kind):
    """Exactly the names of the mask in bit order, with the tables' dtypes and widths, as numpy
    arrays and as torch tensors; the record points at them, NULL for the rest."""
    rows, every = TABLES[kind]
    record = {"DL": capi.DirectLightPtrs, "SC": capi.ScatterPtrs, "CH": capi.ClosestPtrs}[kind]
    assert [n for n, _ in record._fields_] == [r[0] for r in rows]
    n = 5
    for mask in range(1, every + 1):
        want = [(name, np.dtype(dt), (n, k) if k else (n,)) for name, bit, dt, k in rows
                if mask & bit]
        res, ptrs = capi._outputs(kind, mask, n)
        assert isinstance(ptrs, record)
        assert [(k, v.dtype, v.shape) for k, v in res.items()] == want
        tres, tptrs = capi._outputs(kind, mask, n, CPU)
        assert [(k, np.dtype(str(v.dtype).split(".")[-1]), tuple(v.shape))
                for k, v in tres.items()] == want
        for name, *_ in rows:
            assert getattr(ptrs, name) == (res[name].ctypes.data if name in res else None)
            assert getattr(tptrs, name) == (tres[name].data_ptr() if name in tres else None)
    # a given tensor is taken as it is; one element too small is rejected; n = 0 gives no NULL
    name, _, dt, k = rows[-1]
    tdt = getattr(torch, np.dtype(dt).name)
    given = torch.zeros(n * max(k, 1), dtype=tdt)
    res, _ = capi._outputs(kind, every, n, CPU, {name: given})
    assert res[name] is given and list(res) == [r[0] for r in rows]
    with pytest.raises(ValueError, match=rf"out\['{name}'\]: a contiguous .* n\*{max(k, 1)} "):
        capi._outputs(kind, every, n, CPU, {name: given[:-1]})
    for dev in (None, CPU):
        _, ptrs = capi._outputs(kind, every, 0, dev)
        assert all(getattr(ptrs, r[0]) for r in rows)


@pytest.mark.parametrize("check,every", [(capi._dl_check, capi.DL_ALL),
                                         (capi._sc_check, capi.SC_ALL),
                                         (capi._ch_check, capi.CH_ALL)])
def test_mask_checks(check, every):
    for mask in range(1, every + 1):
        check(mask)
    for bad in (0, every + 1, every | (every + 1)):   # none, an unknown bit, ALL | unknown
        with pytest.raises(ValueError, match="outputs: a non-empty combination"):
            check(bad)


@pytest.mark.parametrize("kind", sorted(TABLES))
def test_outputs_checks_the_mask(kind):
    every = TABLES[kind][1]
    for bad in (0, every + 1, every | (every + 1)):
        with pytest.raises(ValueError, match=f"combination of {kind}_"):
            capi._outputs(kind, bad, 4)


def test_query_opts():
    o = capi._query_opts()
    d = capi.default_opts()
    assert (o.flags, o.bias, o.max_recursion) == (0, d.bias, d.max_recursion)
    o = capi._query_opts(2e-3, True, 0)
    assert (o.flags, o.bias, o.max_recursion) == (capi.RT_FLAG_NO_BVH, 2e-3, 0)
    assert capi._query_opts(no_bvh=True).bias == d.bias


def test_device_methods_use_the_helpers():
    """Every *_device method of DeviceScene is there, holds no contiguity check of its own and
    goes through one of the helpers."""
    names = {"occluded_device", "transmittance_device", "light_transmittance_device",
             "direct_light_device", "direct_light_rays_device", "scatter_device",
             "closest_device", "trace_rays_device", "camera_rays_device", "accumulate_device",
             "resolve_device"}
    found = {n for n, f in vars(capi.DeviceScene).items() if n.endswith("_device") and callable(f)}
    assert names <= found, names - found
    for n in sorted(names):
        f = getattr(capi.DeviceScene, n)
        assert "is_contiguous" not in inspect.getsource(f), n
        assert HELPERS & set(f.__code__.co_names), n
    # the input, single-output, output-dict and max_dist helpers hold the only four
    assert inspect.getsource(capi).count("is_contiguous") == 4
