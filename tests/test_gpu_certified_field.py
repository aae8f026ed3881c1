"""Certified distance-field check on the device (mtg_certify_distance_field, csrc/mtg_certify.hip) against the library's host build
of the same lane code: every output bit for bit -- the first 25 trajectories of the four fixture cases under both outside values
and both layouts of the times, a batch whose frontier passes one chunk of 64 nodes, the depth limit and the budget, absent optional
outputs, refused arguments, and the torch form of the Lipschitz helper."""
import ctypes

import numpy as np
import pytest

from test_certified_field import BUDGET, COLLIDES, DEPTH, FREE, field_of, graze_batch, output_shapes
from test_distance_field import CASES, H, INFLATION, field_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import mav_trajectory_generation_amd as m
    c = m.Context(0)
    yield c
    c.close()


def both_forms(ctx, coeffs, times, field, lipschitz, inflation, layout="aos", **limits):
    """(device result as numpy arrays, host result); field: a DistanceField of a numpy grid."""
    import torch
    import mav_trajectory_generation_amd as m
    times = np.asarray(times, dtype=np.float64)
    t = times if layout == "aos" else np.ascontiguousarray(times.T)
    dev = m.DistanceField(torch.from_numpy(np.ascontiguousarray(field.distances)).cuda(), field.origin, field.voxel_size, field.outside_distance)
    out = m.certify_distance_field(ctx, torch.from_numpy(np.array(coeffs, dtype=np.float64)).cuda(), torch.from_numpy(np.array(t)).cuda(), dev,
                                   lipschitz, inflation=inflation, times_layout=layout, **limits)
    ctx.sync()
    d = m.CertifiedFieldResult(*[o.cpu().numpy() for o in out[:11]], out.lipschitz)
    return d, m.certify_distance_field_host(coeffs, t, field, lipschitz, inflation=inflation, times_layout=layout, **limits)


def bit_for_bit(d, h):
    for name, a, b in zip(d._fields[:11], d, h):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert a.tobytes() == b.tobytes(), (name, np.nonzero(a.ravel().view(np.int64 if a.dtype == np.float64 else np.int32)
                                                               != b.ravel().view(np.int64 if b.dtype == np.float64 else np.int32))[0][:8])


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("outside", [0.0, np.inf], ids=["out0", "outinf"])
@pytest.mark.parametrize("name", CASES)
def test_device_equals_host_bit_for_bit(ctx, name, outside, layout):
    """N = 10, 12 and the zero-padded 5 and 7; D = 3 and 4; 200, 75, 100 and 100 segments."""
    coeffs, times, _, _ = field_case(name)
    f, lip = field_of(name, outside)
    d, h = both_forms(ctx, coeffs[:25], times[:25], f, lip, INFLATION, layout)
    print(f"{name} outside={outside} {layout}: verdicts {np.bincount(h.trajectory_result, minlength=4)}, nodes mean {h.segment_nodes.mean():.1f}")
    if outside == np.inf:
        assert (h.trajectory_result == FREE).any() and (h.trajectory_result == COLLIDES).any()
    bit_for_bit(d, h)


def test_a_frontier_beyond_one_chunk_of_64(ctx):
    """B = 3, K = 2 on the d = x field: frontiers of 256 and 512 nodes (the chunk loop), and tilted lines where failing, certified
    and surviving nodes alternate within a chunk (the ordered compaction).  tests/test_certified_field.py checks on the CPU that
    the host form's largest frontier exceeds 64 on it."""
    coeffs, times, f, lip, inflation = graze_batch()
    d, h = both_forms(ctx, coeffs, times, f, lip, inflation, min_depth=0, max_frontier=1024)
    assert h.segment_nodes[:, 0].tolist() == [511, 1023, 1023]
    bit_for_bit(d, h)
    d, h = both_forms(ctx, coeffs, times, f, lip, inflation, min_depth=0, max_frontier=256)
    assert (h.segment_result == BUDGET).sum() == 2
    bit_for_bit(d, h)
    d, h = both_forms(ctx, coeffs, times, f, lip, inflation, min_depth=6, max_depth=6, max_frontier=64)
    assert (h.segment_result == DEPTH).any()
    bit_for_bit(d, h)


@pytest.mark.parametrize("name", CASES)
def test_depth_limit_and_budget(ctx, name):
    coeffs, times, _, _ = field_case(name)
    f, lip = field_of(name, np.inf)
    d, h = both_forms(ctx, coeffs[:25], times[:25], f, lip, INFLATION, min_depth=0, max_depth=3)
    assert (h.segment_result == DEPTH).sum() >= 48
    bit_for_bit(d, h)
    d, h = both_forms(ctx, coeffs[:25], times[:25], f, lip, INFLATION, min_depth=0, max_frontier=4)
    assert (h.segment_result == BUDGET).sum() >= 33 and (d.segment_lower_bound[h.segment_result == BUDGET] == -np.inf).all()
    bit_for_bit(d, h)


def test_segment_times_that_are_not_positive_and_nan(ctx):
    coeffs, times, _, _ = field_case("n7_k4_d4")
    f, lip = field_of("n7_k4_d4", np.inf)
    coeffs, times = coeffs[:6].copy(), times[:6].copy()
    times[0, 1], times[1, 0], times[2, 3] = 0.0, -0.5, np.nan
    coeffs[3, 2, 1, 2] = np.nan
    coeffs[4, :, 3] = np.nan                                                    # yaw: never read
    d, h = both_forms(ctx, coeffs, times, f, lip, INFLATION)
    assert h.segment_nodes[0, 1] == 1 and h.segment_result[2, 3] == COLLIDES and np.isnan(h.segment_lower_bound[3, 2])
    bit_for_bit(d, h)


def raw_device_call(ctx, co, ti, fc, lip, limits, inflation, outs):
    b, k, d, n = co.shape
    return ctx.lib.mtg_certify_distance_field(ctx.handle, n, k, d, b, co.data_ptr(), ti.data_ptr(), k, 1, ctypes.byref(fc), lip, *limits, inflation,
                                              *[None if o is None else o.data_ptr() for o in outs])


def test_optional_outputs_absent_and_refused_arguments(ctx):
    import torch
    from mav_trajectory_generation_amd import _lib as L
    coeffs, times, grid, origin = field_case("n5_k3_d3")
    _, lip = field_of("n5_k3_d3", 0.0)
    co, ti, gr = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (coeffs[:9], times[:9], grid))
    fc = L.DistanceFieldC(gr.data_ptr(), grid.shape[2], grid.shape[1], grid.shape[0], (ctypes.c_double * 3)(*origin), H, 0.0, 1)
    b, k = ti.shape
    GUARD, limits = 3, (4, 16, 1024)
    torch_type = {np.int32: torch.int32, np.float64: torch.float64}

    def buffers():
        return [torch.full((int(np.prod(s)) + 2 * GUARD,), -77, dtype=torch_type[dt], device="cuda") for s, dt in output_shapes(b, k)]
    full = buffers()
    assert raw_device_call(ctx, co, ti, fc, lip, limits, INFLATION, [a[GUARD:] for a in full]) == 0
    ctx.sync()
    full = [a.cpu().numpy() for a in full]
    for a in full:                                    # written in full, and not beyond
        assert (a[:GUARD] == -77).all() and (a[-GUARD:] == -77).all() and not (a[GUARD:-GUARD] == -77).any()
    for present in ([False] * 10, [True, False] * 5, [False, True] * 5, [False] * 8 + [True, True], [True] + [False] * 9):
        some = buffers()
        outs = [some[0][GUARD:]] + [some[i + 1][GUARD:] if p else None for i, p in enumerate(present)]
        assert raw_device_call(ctx, co, ti, fc, lip, limits, INFLATION, outs) == 0
        ctx.sync()
        for i, (a, ref) in enumerate(zip(some, full)):
            a = a.cpu().numpy()
            assert np.array_equal(a, ref, equal_nan=True) if (i == 0 or present[i - 1]) else (a == -77).all()
    # refused: MTG_ERR_INVALID_ARGUMENT, nothing enqueued, every output untouched
    near = L.DistanceFieldC(gr.data_ptr(), grid.shape[2], grid.shape[1], grid.shape[0], (ctypes.c_double * 3)(*origin), H, 0.0, 0)
    for field, l, lim in ((near, lip, limits), (fc, 0.0, limits), (fc, float("inf"), limits), (fc, float("nan"), limits), (fc, lip, (11, 16, 1024)),
                          (fc, lip, (4, 3, 1024)), (fc, lip, (4, 25, 1024)), (fc, lip, (4, 16, 15)), (fc, lip, (4, 16, 1025)), (fc, lip, (-1, 16, 1024))):
        some = buffers()
        assert raw_device_call(ctx, co, ti, field, l, lim, INFLATION, [a[GUARD:] for a in some]) == -1
        assert b"certified distance field" in ctx.lib.mtg_last_error_string(ctx.handle)
        ctx.sync()
        assert all((a.cpu().numpy() == -77).all() for a in some)
    some = buffers()
    assert ctx.lib.mtg_certify_distance_field(ctx.handle, 5, 3, 3, 0, co.data_ptr(), ti.data_ptr(), 3, 1, ctypes.byref(fc), lip, *limits, INFLATION,
                                              *[a[GUARD:].data_ptr() for a in some]) == 0                          # batch = 0
    ctx.sync()
    assert all((a.cpu().numpy() == -77).all() for a in some)


def test_want_segments_false_and_single_calls(ctx):
    import torch
    import mav_trajectory_generation_amd as m
    coeffs, times, grid, origin = field_case("n12_k4_d4")
    f, lip = field_of("n12_k4_d4", np.inf)
    dev = m.DistanceField(torch.from_numpy(grid).cuda(), origin, H, np.inf)
    co, ti = torch.from_numpy(coeffs[:25]).cuda(), torch.from_numpy(times[:25]).cuda()
    r = m.certify_distance_field(ctx, co, ti, dev, lip, inflation=INFLATION, want_segments=False)
    ctx.sync()
    h = m.certify_distance_field_host(coeffs[:25], times[:25], f, lip, inflation=INFLATION)
    assert all(x is None for x in r[2:9])
    for i in (0, 1, 9, 10):
        assert r[i].cpu().numpy().tobytes() == h[i].tobytes()
    # lipschitz = None computes the torch bound, which is at or above the host's
    r = m.certify_distance_field(ctx, co, ti, dev, inflation=INFLATION)
    ctx.sync()
    assert lip <= r.lipschitz <= lip * (1.0 + 1e-12)


@pytest.mark.parametrize("name", CASES)
def test_torch_lipschitz_bound(ctx, name):
    import torch
    import mav_trajectory_generation_amd as m
    _, _, grid, origin = field_case(name)
    host = field_of(name, 0.0)[1]
    dev = m.DistanceField(torch.from_numpy(grid).cuda(), origin, H).lipschitz_bound()
    print(f"{name}: host {host!r}, torch {dev!r}, relative difference {(dev - host) / host:.3e}")
    assert host <= dev <= host * (1.0 + 1e-12)
    bad = grid.copy()
    bad[2, 3, 4] = np.nan
    assert not np.isfinite(m.DistanceField(torch.from_numpy(bad).cuda(), origin, H).lipschitz_bound())
