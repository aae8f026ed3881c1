"""Argument table of mtg_check_distance_field_host and (marked gpu) mtg_check_distance_field: one row per error of
include/mtg_hip.h -- the shape rules the per-segment entries share, this entry's own limits (N 1 .. 12, D 3 or 4, fewer than 2^19
segments), the field (dims, voxel count, voxel_size, origin, outside_distance, interpolation), dt, max_samples, inflation and
the required pointers -- and the Python layer's own errors, which come before any allocation.  Return codes only."""
import ctypes

import numpy as np
import pytest

import mav_trajectory_generation_amd as m
from mav_trajectory_generation_amd import _lib as L

OK, INVALID = 0, -1
B, K = 3, 4
NAN, INF = float("nan"), float("inf")

# (id, N, K, D, batch, ts_b, ts_k, expected)
SHAPE_CASES = [
    ("n_0", 0, K, 3, B, K, 1, INVALID), ("n_1", 1, K, 3, B, K, 1, OK), ("n_odd", 7, K, 3, B, K, 1, OK), ("n_12", 12, K, 3, B, K, 1, OK),
    ("n_13", 13, K, 3, B, K, 1, INVALID), ("k_0", 10, 0, 3, B, 1, 1, INVALID), ("k_1", 10, 1, 3, B, 1, 1, OK),
    ("d_2", 10, K, 2, B, K, 1, INVALID), ("d_3", 10, K, 3, B, K, 1, OK), ("d_4", 10, K, 4, B, K, 1, OK), ("d_5", 10, K, 5, B, K, 1, INVALID),
    ("batch_minus_1", 10, K, 3, -1, K, 1, INVALID), ("batch_0", 10, K, 3, 0, K, 1, OK), ("ts_b_0", 10, K, 3, B, 0, 1, INVALID),
    ("ts_k_0", 10, K, 3, B, K, 0, INVALID), ("rows_bk_overlapping", 10, K, 3, B, K * 2 - 1, 2, INVALID),
    ("rows_bk_padded", 10, K, 3, B, K * 2 + 3, 2, OK), ("rows_kb_overlapping", 10, K, 3, B, 2, B * 2 - 1, INVALID), ("soa", 10, K, 3, B, 1, B, OK),
]

# (id, overrides of the accepted call, expected); dims = (nx, ny, nz); with batch = 0 the grid is never read
FIELD_CASES = [
    ("accepted", {}, OK),
    ("nx_1_trilinear", dict(dims=(1, 4, 4)), INVALID), ("ny_1_trilinear", dict(dims=(4, 1, 4)), INVALID),
    ("nz_1_trilinear", dict(dims=(4, 4, 1)), INVALID), ("nx_2_trilinear", dict(dims=(2, 2, 2)), OK),
    ("n_1_nearest", dict(dims=(1, 1, 1), interpolation=0), OK), ("nx_0_nearest", dict(dims=(0, 4, 4), interpolation=0), INVALID),
    ("ny_negative", dict(dims=(4, -4, 4)), INVALID), ("nz_0_nearest", dict(dims=(4, 4, 0), interpolation=0), INVALID),
    ("voxels_2^31", dict(dims=(2048, 2048, 512), batch=0), INVALID), ("voxels_2^31-2048", dict(dims=(2047, 2048, 512), batch=0), OK),
    ("voxels_wrap_int32", dict(dims=(65536, 65536, 2), batch=0), INVALID), ("voxels_nx_ny_2^62", dict(dims=(1 << 30, 1 << 30, 2), batch=0), INVALID),
    ("voxel_size_0", dict(voxel_size=0.0), INVALID), ("voxel_size_negative", dict(voxel_size=-0.5), INVALID),
    ("voxel_size_nan", dict(voxel_size=NAN), INVALID), ("voxel_size_inf", dict(voxel_size=INF), INVALID),
    ("voxel_size_reciprocal_overflows", dict(voxel_size=5e-324), INVALID), ("voxel_size_small", dict(voxel_size=1e-300), OK),
    ("origin_nan", dict(origin=(0.0, NAN, 0.0)), INVALID), ("origin_inf", dict(origin=(0.0, 0.0, -INF)), INVALID),
    ("origin_x_inf", dict(origin=(INF, 0.0, 0.0)), INVALID),
    ("outside_nan", dict(outside=NAN), INVALID), ("outside_inf", dict(outside=INF), OK), ("outside_minus_inf", dict(outside=-INF), OK),
    ("outside_negative", dict(outside=-3.0), OK),
    ("interpolation_2", dict(interpolation=2), INVALID), ("interpolation_negative", dict(interpolation=-1), INVALID),
    ("dt_0", dict(dt=0.0), INVALID), ("dt_negative", dict(dt=-0.1), INVALID), ("dt_nan", dict(dt=NAN), INVALID), ("dt_inf", dict(dt=INF), INVALID),
    ("dt_tiny", dict(dt=5e-324), OK),
    ("max_samples_1", dict(max_samples=1), INVALID), ("max_samples_2", dict(max_samples=2), OK), ("max_samples_0", dict(max_samples=0), INVALID),
    ("max_samples_2^20", dict(max_samples=1 << 20), OK), ("max_samples_2^20+1", dict(max_samples=(1 << 20) + 1), INVALID),
    ("inflation_negative", dict(inflation=-1e-300), INVALID), ("inflation_nan", dict(inflation=NAN), INVALID),
    ("inflation_inf", dict(inflation=INF), INVALID),
    ("null_coeffs", dict(null="coeffs"), INVALID), ("null_times", dict(null="times"), INVALID), ("null_field", dict(null="field"), INVALID),
    ("null_distances", dict(null="distances"), INVALID), ("null_feasible", dict(null="feasible"), INVALID),
]


def arguments(n, k, d, batch, ts_b, ts_k, dims=(4, 3, 2), voxel_size=0.5, origin=(0.0, 0.0, 0.0), outside=0.0, interpolation=1, dt=0.25,
              max_samples=64, inflation=0.0):
    """numpy buffers of an accepted reading of the arguments: (coeffs, times, grid, feasible)."""
    nb, nk, nd, nn = max(batch, 1), max(k, 1), max(d, 1), max(n, 1)
    coeffs = np.random.default_rng(1000 * nn + nd).standard_normal((nb, nk, nd, nn))
    times = np.ones(((nb - 1) * max(ts_b, 0) + (nk - 1) * max(ts_k, 0) + 1,))
    voxels = int(np.prod([max(x, 1) for x in dims]))
    grid = np.ones((voxels if voxels <= 4096 else 8,), dtype=np.float32)
    return coeffs, times, grid, np.full((nb,), -7, dtype=np.int32)


def host_call(n, k, d, batch, ts_b, ts_k, null=None, **o):
    coeffs, times, grid, feas = arguments(n, k, d, batch, ts_b, ts_k, **o)
    dims = o.get("dims", (4, 3, 2))
    fc = L.DistanceFieldC(None if null == "distances" else grid.ctypes.data, dims[0], dims[1], dims[2],
                          (ctypes.c_double * 3)(*o.get("origin", (0.0, 0.0, 0.0))), o.get("voxel_size", 0.5), o.get("outside", 0.0),
                          o.get("interpolation", 1))
    ptr = {"coeffs": coeffs.ctypes.data, "times": times.ctypes.data, "field": ctypes.byref(fc), "feasible": feas.ctypes.data}
    if null in ptr:
        ptr[null] = None
    rc = L.load().mtg_check_distance_field_host(n, k, d, batch, ptr["coeffs"], ptr["times"], ts_b, ts_k, ptr["field"], o.get("dt", 0.25),
                                                o.get("max_samples", 64), o.get("inflation", 0.0), ptr["feasible"], None, None, None, None,
                                                None, None)
    if rc != OK or batch == 0:
        assert (feas == -7).all()
    return rc


@pytest.mark.parametrize("case", SHAPE_CASES, ids=[c[0] for c in SHAPE_CASES])
def test_shape_rules(case):
    name, n, k, d, batch, ts_b, ts_k, expected = case
    assert host_call(n, k, d, batch, ts_b, ts_k) == expected, case


@pytest.mark.parametrize("case", FIELD_CASES, ids=[c[0] for c in FIELD_CASES])
def test_field_and_sampling_rules(case):
    name, o, expected = case
    o = dict(o)
    assert host_call(10, K, 3, o.pop("batch", B), K, 1, **o) == expected, case


def test_segment_count_limit_of_the_failure_word():
    lib = L.load()
    one = np.ones(8, dtype=np.float64)
    grid = np.ones(8, dtype=np.float32)
    fc = L.DistanceFieldC(grid.ctypes.data, 2, 2, 2, (ctypes.c_double * 3)(0, 0, 0), 0.5, 0.0, 1)
    out = np.empty((1,), dtype=np.int32)
    args = (3, 0, one.ctypes.data, one.ctypes.data, 1 << 19, 1, ctypes.byref(fc), 0.25, 64, 0.0, out.ctypes.data, None, None, None, None, None, None)
    assert lib.mtg_check_distance_field_host(10, 1 << 19, *args) == INVALID
    assert lib.mtg_check_distance_field_host(10, (1 << 19) - 1, *args) == OK


class NoAllocation:
    """A _SegmentBatch whose `empty` must not be reached."""


def test_python_layer_errors_come_before_any_allocation(monkeypatch):
    from mav_trajectory_generation_amd import segment_checks as sc
    coeffs, times = np.zeros((2, 3, 3, 4)), np.ones((2, 3))
    grid = np.ones((4, 3, 2), dtype=np.float32)
    good = m.DistanceField(grid, (0.0, 0.0, 0.0), 0.5)
    assert m.check_distance_field_host(coeffs, times, good, 0.25).trajectory_feasible.tolist() == [1, 1]

    def no_empty(self, *a, **k):
        raise AssertionError("an output was allocated before the arguments were checked")
    monkeypatch.setattr(sc._SegmentBatch, "empty", no_empty)
    for bad in (m.DistanceField(grid.astype(np.float64), (0.0, 0.0, 0.0), 0.5),            # dtype
                m.DistanceField(grid[0], (0.0, 0.0, 0.0), 0.5),                              # rank
                m.DistanceField(grid[None], (0.0, 0.0, 0.0), 0.5),
                m.DistanceField(grid[:, :, ::2], (0.0, 0.0, 0.0), 0.5),                      # not contiguous
                m.DistanceField(grid.tolist(), (0.0, 0.0, 0.0), 0.5),                        # not an array
                m.DistanceField(np.ones((0, 3, 2), dtype=np.float32), (0.0, 0.0, 0.0), 0.5),
                (grid, (0.0, 0.0, 0.0), 0.5)):                                               # not a DistanceField
        with pytest.raises(m.MtgError) as e:
            m.check_distance_field_host(coeffs, times, bad, 0.25)
        assert e.value.code == -1
    for origin in ((0.0, 0.0), (0.0, 0.0, 0.0, 0.0), 0.0, ()):
        with pytest.raises(m.MtgError):
            m.DistanceField(grid, origin, 0.5)
        with pytest.raises(m.MtgError):
            m.DistanceField.from_corner(grid, origin, 0.5)
    with pytest.raises(m.MtgError):
        m.DistanceField(grid, (0.0, 0.0, 0.0), 0.5, interpolation="cubic")


def test_library_errors_reach_python_as_mtg_error():
    coeffs, times = np.zeros((2, 3, 3, 4)), np.ones((2, 3))
    grid = np.ones((4, 3, 2), dtype=np.float32)
    good = m.DistanceField(grid, (0.0, 0.0, 0.0), 0.5)
    for kw in (dict(dt=0.0), dict(dt=0.25, inflation=-1.0), dict(dt=0.25, max_samples=1), dict(dt=0.25, max_samples=(1 << 20) + 1)):
        with pytest.raises(m.MtgError):
            m.check_distance_field_host(coeffs, times, good, **kw)
    for bad in (m.DistanceField(grid, (0.0, 0.0, 0.0), 0.0), m.DistanceField(grid, (0.0, NAN, 0.0), 0.5),
                m.DistanceField(grid, (0.0, 0.0, 0.0), 0.5, outside_distance=NAN), m.DistanceField(grid[:, :, :1].copy(), (0.0, 0.0, 0.0), 0.5)):
        with pytest.raises(m.MtgError):
            m.check_distance_field_host(coeffs, times, bad, 0.25)


# ---- the same table on the device entry ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = m.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
def test_device_entry_table(ctx):
    """Every row of both tables in one test (one context, one set of buffers per row): the return code, the context's message, and
    nothing enqueued on a refusal -- trajectory_feasible keeps its guard value."""
    import torch
    rows = [(c[0], c[1:7], {}, c[7]) for c in SHAPE_CASES] + [(c[0], (10, K, 3, B, K, 1), c[1], c[2]) for c in FIELD_CASES]
    for name, shape, o, expected in rows:
        o = dict(o)
        null = o.pop("null", None)
        n, k, d, batch, ts_b, ts_k = shape
        batch = o.pop("batch", batch)
        coeffs, times, grid, feas = arguments(n, k, d, batch, ts_b, ts_k, **o)
        co, ti, gr, fe = (torch.from_numpy(a).cuda() for a in (coeffs, times, grid, feas))
        dims = o.get("dims", (4, 3, 2))
        fc = L.DistanceFieldC(None if null == "distances" else gr.data_ptr(), dims[0], dims[1], dims[2],
                              (ctypes.c_double * 3)(*o.get("origin", (0.0, 0.0, 0.0))), o.get("voxel_size", 0.5), o.get("outside", 0.0),
                              o.get("interpolation", 1))
        ptr = {"coeffs": co.data_ptr(), "times": ti.data_ptr(), "field": ctypes.byref(fc), "feasible": fe.data_ptr()}
        if null in ptr:
            ptr[null] = None
        torch.cuda.synchronize()
        rc = ctx.lib.mtg_check_distance_field(ctx.handle, n, k, d, batch, ptr["coeffs"], ptr["times"], ts_b, ts_k, ptr["field"],
                                              o.get("dt", 0.25), o.get("max_samples", 64), o.get("inflation", 0.0), ptr["feasible"], None, None,
                                              None, None, None, None)
        ctx.sync()
        assert rc == expected, name
        if rc != OK:
            assert b"distance field" in ctx.lib.mtg_last_error_string(ctx.handle), name
        if rc != OK or batch == 0:
            assert (fe.cpu().numpy() == -7).all(), name
    assert ctx.lib.mtg_check_distance_field(None, 10, K, 3, B, 1, 1, K, 1, None, 0.25, 64, 0.0, 1, None, None, None, None, None, None) == INVALID


@pytest.mark.gpu
def test_python_layer_errors_on_the_device_form(ctx, monkeypatch):
    import torch
    from mav_trajectory_generation_amd import segment_checks as sc
    coeffs, times = torch.zeros((2, 3, 3, 4), dtype=torch.float64, device="cuda"), torch.ones((2, 3), dtype=torch.float64, device="cuda")
    grid = torch.ones((4, 3, 2), dtype=torch.float32, device="cuda")
    assert m.check_distance_field(ctx, coeffs, times, m.DistanceField(grid, (0.0, 0.0, 0.0), 0.5), 0.25).trajectory_feasible.tolist() == [1, 1]

    def no_empty(self, *a, **k):
        raise AssertionError("an output was allocated before the arguments were checked")
    monkeypatch.setattr(sc._SegmentBatch, "empty", no_empty)
    for bad in (grid.double(), grid[0], grid[:, :, ::2], grid.cpu(), grid.cpu().numpy()):
        with pytest.raises(m.MtgError) as e:
            m.check_distance_field(ctx, coeffs, times, m.DistanceField(bad, (0.0, 0.0, 0.0), 0.5), 0.25)
        assert e.value.code == -1
