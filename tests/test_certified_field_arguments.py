"""Argument table of mtg_certify_distance_field_host and (marked gpu) mtg_certify_distance_field: the sampled check's rows
(tests/test_distance_field_arguments.py: the shared shape rules and the field's, without dt and max_samples; a nearest field is
now refused), and this entry's own: lipschitz, min_depth, max_depth, max_frontier and the required pointers.  Return codes only."""
import ctypes

import numpy as np
import pytest

import mav_trajectory_generation_amd as m
from mav_trajectory_generation_amd import _lib as L
from test_distance_field_arguments import B, FIELD_CASES, INF, INVALID, K, NAN, OK, SHAPE_CASES, arguments

# the sampled check's field rows that exist here; a row that asks for a nearest field is an error whatever else it holds
FIELD_ROWS = [(name, o, INVALID if o.get("interpolation") == 0 else expected) for name, o, expected in FIELD_CASES
              if not ({"dt", "max_samples"} & set(o)) and o.get("null") != "feasible"]
OWN_ROWS = [
    ("nearest", dict(interpolation=0), INVALID),
    ("lipschitz_0", dict(lipschitz=0.0), INVALID), ("lipschitz_negative", dict(lipschitz=-1.0), INVALID),
    ("lipschitz_nan", dict(lipschitz=NAN), INVALID), ("lipschitz_inf", dict(lipschitz=INF), INVALID),
    ("lipschitz_tiny", dict(lipschitz=5e-324), OK), ("lipschitz_huge", dict(lipschitz=1e308), OK),
    ("min_depth_negative", dict(min_depth=-1), INVALID), ("min_depth_0", dict(min_depth=0), OK),
    ("min_depth_10", dict(min_depth=10, max_frontier=1024), OK), ("min_depth_11", dict(min_depth=11, max_depth=16, max_frontier=1024), INVALID),
    ("max_depth_below_min", dict(min_depth=4, max_depth=3), INVALID), ("max_depth_equals_min", dict(min_depth=4, max_depth=4), OK),
    ("max_depth_24", dict(max_depth=24), OK), ("max_depth_25", dict(max_depth=25), INVALID),
    ("max_frontier_below_2^min_depth", dict(min_depth=4, max_frontier=15), INVALID), ("max_frontier_2^min_depth", dict(min_depth=4, max_frontier=16), OK),
    ("max_frontier_1", dict(min_depth=0, max_frontier=1), INVALID), ("max_frontier_2", dict(min_depth=0, max_frontier=2), OK),
    ("max_frontier_2_min_depth_1", dict(min_depth=1, max_frontier=2), OK), ("max_frontier_1024", dict(max_frontier=1024), OK),
    ("max_frontier_1025", dict(max_frontier=1025), INVALID), ("max_frontier_0", dict(min_depth=0, max_frontier=0), INVALID),
    ("null_result", dict(null="result"), INVALID),
]
OWN_KEYS = ("lipschitz", "min_depth", "max_depth", "max_frontier")


def split(o):
    """(the overrides `arguments` knows, lipschitz, (min_depth, max_depth, max_frontier), inflation)."""
    o = dict(o)
    own = {k: o.pop(k) for k in OWN_KEYS if k in o}
    limits = (own.get("min_depth", 4), own.get("max_depth", 16), own.get("max_frontier", 1024))
    return o, own.get("lipschitz", 1.5), limits, o.get("inflation", 0.0)


def field_struct(o, null, address):
    dims = o.get("dims", (4, 3, 2))
    return L.DistanceFieldC(None if null == "distances" else address, dims[0], dims[1], dims[2], (ctypes.c_double * 3)(*o.get("origin", (0.0, 0.0, 0.0))),
                            o.get("voxel_size", 0.5), o.get("outside", 0.0), o.get("interpolation", 1))


def host_call(n, k, d, batch, ts_b, ts_k, null=None, **o):
    o, lipschitz, limits, inflation = split(o)
    coeffs, times, grid, result = arguments(n, k, d, batch, ts_b, ts_k, **o)
    fc = field_struct(o, null, grid.ctypes.data)
    ptr = {"coeffs": coeffs.ctypes.data, "times": times.ctypes.data, "field": ctypes.byref(fc), "result": result.ctypes.data}
    if null in ptr:
        ptr[null] = None
    rc = L.load().mtg_certify_distance_field_host(n, k, d, batch, ptr["coeffs"], ptr["times"], ts_b, ts_k, ptr["field"], lipschitz, *limits,
                                                  inflation, ptr["result"], *[None] * 10)
    if rc != OK or batch == 0:
        assert (result == -7).all()
    else:
        assert np.isin(result[:batch], (0, 1, 2, 3)).all()
    return rc


@pytest.mark.parametrize("case", SHAPE_CASES, ids=[c[0] for c in SHAPE_CASES])
def test_shape_rules(case):
    name, n, k, d, batch, ts_b, ts_k, expected = case
    assert host_call(n, k, d, batch, ts_b, ts_k) == expected, case


@pytest.mark.parametrize("case", FIELD_ROWS + OWN_ROWS, ids=[c[0] for c in FIELD_ROWS + OWN_ROWS])
def test_field_and_search_rules(case):
    name, o, expected = case
    o = dict(o)
    assert host_call(10, K, 3, o.pop("batch", B), K, 1, **o) == expected, case


def test_segment_count_limit_of_the_failure_word():
    lib = L.load()
    one = np.ones(8, dtype=np.float64)
    grid = np.ones(8, dtype=np.float32)
    fc = L.DistanceFieldC(grid.ctypes.data, 2, 2, 2, (ctypes.c_double * 3)(0, 0, 0), 0.5, 0.0, 1)
    out = np.empty((1,), dtype=np.int32)
    args = (3, 0, one.ctypes.data, one.ctypes.data, 1 << 19, 1, ctypes.byref(fc), 1.0, 4, 16, 1024, 0.0, out.ctypes.data) + (None,) * 10
    assert lib.mtg_certify_distance_field_host(10, 1 << 19, *args) == INVALID
    assert lib.mtg_certify_distance_field_host(10, (1 << 19) - 1, *args) == OK


def test_python_layer_errors():
    coeffs, times = np.zeros((2, 3, 3, 4)), np.ones((2, 3))
    grid = np.ones((4, 3, 2), dtype=np.float32)
    grid[1, 1, 1] = 1.5
    good = m.DistanceField(grid, (0.0, 0.0, 0.0), 0.5)
    assert m.certify_distance_field_host(coeffs, times, good).trajectory_result.tolist() == [1, 1]
    for bad in (m.DistanceField(grid.astype(np.float64), (0.0, 0.0, 0.0), 0.5), m.DistanceField(grid[0], (0.0, 0.0, 0.0), 0.5),
                m.DistanceField(grid[:, :, ::2], (0.0, 0.0, 0.0), 0.5), m.DistanceField(grid.tolist(), (0.0, 0.0, 0.0), 0.5),
                (grid, (0.0, 0.0, 0.0), 0.5)):
        with pytest.raises(m.MtgError) as e:
            m.certify_distance_field_host(coeffs, times, bad, 1.0)
        assert e.value.code == -1
    for kw in (dict(lipschitz=0.0), dict(lipschitz=NAN), dict(lipschitz=INF), dict(inflation=-1.0), dict(min_depth=11), dict(max_depth=3),
               dict(max_depth=25), dict(max_frontier=15), dict(max_frontier=1025)):
        with pytest.raises(m.MtgError):
            m.certify_distance_field_host(coeffs, times, good, **kw)
    with pytest.raises(m.MtgError):
        m.certify_distance_field_host(coeffs, times, m.DistanceField(grid, (0.0, 0.0, 0.0), 0.5, interpolation="nearest"), 1.0)
    with pytest.raises(m.MtgError):                                             # a constant grid: L = 0 is not a promise the check takes
        m.certify_distance_field_host(coeffs, times, m.DistanceField(np.ones((4, 3, 2), dtype=np.float32), (0.0, 0.0, 0.0), 0.5))


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
    """Every row of the tables in one test: the return code, the context's message, and nothing enqueued on a refusal --
    trajectory_result keeps its guard value."""
    import torch
    rows = [(c[0], c[1:7], {}, c[7]) for c in SHAPE_CASES] + [(c[0], (10, K, 3, B, K, 1), c[1], c[2]) for c in FIELD_ROWS + OWN_ROWS]
    for name, shape, o, expected in rows:
        o = dict(o)
        null = o.pop("null", None)
        n, k, d, batch, ts_b, ts_k = shape
        batch = o.pop("batch", batch)
        o, lipschitz, limits, inflation = split(o)
        coeffs, times, grid, result = arguments(n, k, d, batch, ts_b, ts_k, **o)
        co, ti, gr, re = (torch.from_numpy(a).cuda() for a in (coeffs, times, grid, result))
        fc = field_struct(o, null, gr.data_ptr())
        ptr = {"coeffs": co.data_ptr(), "times": ti.data_ptr(), "field": ctypes.byref(fc), "result": re.data_ptr()}
        if null in ptr:
            ptr[null] = None
        torch.cuda.synchronize()
        rc = ctx.lib.mtg_certify_distance_field(ctx.handle, n, k, d, batch, ptr["coeffs"], ptr["times"], ts_b, ts_k, ptr["field"], lipschitz,
                                                *limits, inflation, ptr["result"], *[None] * 10)
        ctx.sync()
        assert rc == expected, name
        if rc != OK:
            assert b"certified distance field" in ctx.lib.mtg_last_error_string(ctx.handle), name
        if rc != OK or batch == 0:
            assert (re.cpu().numpy() == -7).all(), name
    assert ctx.lib.mtg_certify_distance_field(None, 10, K, 3, B, 1, 1, K, 1, None, 1.0, 4, 16, 1024, 0.0, 1, *[None] * 10) == INVALID
