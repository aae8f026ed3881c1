"""Distance-field clearance check on the device (mtg_check_distance_field, csrc/mtg_field.hip): the cases of
tests/test_distance_field.py against the longdouble reference (tests/distance_field_ref.py) under the same rules and against the
library's host build of the same lane code (integers bit for bit, clearances within 2 tol), every instantiation under every
setting of the "field_lanes" knob, the trajectory atomics, graph capture, grid sizes, and the context's status word."""
import ctypes

import numpy as np
import pytest

import distance_field_ref as R
from test_distance_field import (CASES, DT, H, INFLATION, MODE_IDS, MODES, compare, compare_with_reference, field_case, linear_field, line,
                                 reference_of)

pytestmark = pytest.mark.gpu
INTEGERS = ("trajectory_feasible", "first_failing_segment", "segment_closest_sample", "segment_first_failing_sample", "segment_samples")


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import mav_trajectory_generation_amd as m
    c = m.Context(0)
    yield c
    c.close()


def on_device(ctx, coeffs, times, field, dt, inflation=0.0, layout="aos", lanes=0, **kw):
    """field: a DistanceField of a numpy grid; the result as numpy arrays."""
    import torch
    import mav_trajectory_generation_amd as m
    times = np.asarray(times, dtype=np.float64)
    t = times if layout == "aos" else np.ascontiguousarray(times.T)
    dev = m.DistanceField(torch.from_numpy(np.ascontiguousarray(field.distances)).cuda(), field.origin, field.voxel_size,
                          field.outside_distance, field.interpolation)
    ctx.set_option("field_lanes", lanes)
    try:
        out = m.check_distance_field(ctx, torch.from_numpy(np.array(coeffs, dtype=np.float64)).cuda(), torch.from_numpy(np.array(t)).cuda(),
                                     dev, dt, inflation=inflation, times_layout=layout, **kw)
        ctx.sync()
    finally:
        ctx.set_option("field_lanes", 0)
    return m.DistanceFieldResult(*[o.cpu().numpy() if o is not None else None for o in out])


def same_as_host(d, h, seg_tol):
    """Integers bit for bit, clearances within 2 tol (each form is within tol of the exact value)."""
    for name in INTEGERS:
        assert np.array_equal(getattr(d, name), getattr(h, name)), name
    for a, b, tol in ((d.segment_clearance, h.segment_clearance, seg_tol), (d.trajectory_clearance, h.trajectory_clearance, seg_tol.max(axis=1))):
        fin = np.isfinite(b)
        assert np.array_equal(a[~fin], b[~fin], equal_nan=True)
        err = np.abs(a[fin] - b[fin])
        print(f"  device vs host: largest difference {err.max() if err.size else 0.0:.3e}")
        assert (err <= 2.0 * tol[fin]).all()
    assert np.array_equal(d.segment_closest_time, h.segment_closest_time, equal_nan=True)
    assert np.array_equal(d.first_failing_time, h.first_failing_time, equal_nan=True)


def check_everything(ctx, coeffs, times, field, dt, inflation, **kw):
    """The device result against the reference and against the host form; returns it."""
    import mav_trajectory_generation_amd as m
    ref = R.reference(coeffs, times, field.distances, field.origin, field.voxel_size, field.outside_distance, field.interpolation, dt, inflation)
    d = on_device(ctx, coeffs, times, field, dt, inflation, **kw)
    compare(ref, R.expected(ref), np.asarray(times), dt, field.interpolation, d)
    same_as_host(d, m.check_distance_field_host(coeffs, times, field, dt, inflation=inflation), np.where(ref["valid"], ref["tol"], 0.0).max(axis=2))
    return d


@pytest.mark.parametrize("outside,interpolation", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", CASES)
def test_device_entry_vs_reference_and_host(ctx, name, outside, interpolation):
    """N = 10, 12 and the zero-padded 5 and 7; B x K = 800, 120, 240, 160 segments; D = 3 and 4; times as [K][B] in the nearest
    modes."""
    import mav_trajectory_generation_amd as m
    coeffs, times, grid, origin = field_case(name)
    field = m.DistanceField(grid, origin, H, outside, interpolation)
    d = on_device(ctx, coeffs, times, field, DT, INFLATION, layout="soa" if interpolation == "nearest" else "aos")
    compare_with_reference(name, outside, interpolation, d)
    ref, _ = reference_of(name, outside, interpolation)
    same_as_host(d, m.check_distance_field_host(coeffs, times, field, DT, inflation=INFLATION), np.where(ref["valid"], ref["tol"], 0.0).max(axis=2))


SAMPLE_COUNTS = [2, 63, 64, 65, 131, 3, 17, 4, 33, 5, 16, 100, 15]      # G - 1, G, G + 1 and 2 G + 3 for G = 64 (and 4, 16) among them


def instantiation_case(n, d):
    """13 x 5 = 65 segments (with G = 1 one full workgroup plus one lane; with G = 64 the last group alone in its workgroup) with
    the sample counts above, dt = 0.01: slow curves around the centre of a grid with one sphere."""
    rng = np.random.default_rng(100 * n + d)
    coeffs = rng.uniform(-0.6, 0.6, (13, 5, d, n)) / (1.0 + np.arange(n)) ** 2
    coeffs[:, :, :3, 0] = rng.uniform(2.0, 6.0, (13, 5, 3))
    s = np.array([SAMPLE_COUNTS[(i * 5 + k) % 13] for i in range(13) for k in range(5)]).reshape(13, 5)
    s[12, 4] = 131
    times = (s - 1.5) * 0.01
    grid = R.spheres_field((0.0, 0.0, 0.0), (35, 33, 31), 0.25, [[4.0, 4.0, 4.0], [2.5, 5.0, 3.0]], [1.0, 0.6])
    return coeffs, times, s, grid


@pytest.mark.parametrize("d", [3, 4])
@pytest.mark.parametrize("n", range(4, 13))
def test_every_instantiation_and_every_group_size(ctx, n, d):
    """Every output is bit-identical under "field_lanes" = 1, 4, 16, 64 and the default: the fold is a minimum over values that
    each lane computes with the same instructions."""
    import mav_trajectory_generation_amd as m
    coeffs, times, s, grid = instantiation_case(n, d)
    field = m.DistanceField(grid, (0.0, 0.0, 0.0), 0.25, 0.1)
    base = check_everything(ctx, coeffs, times, field, 0.01, 0.3)
    assert np.array_equal(base.segment_samples, s) and 0 < base.trajectory_feasible.sum() < 13
    for lanes in (1, 4, 16, 64, 7):          # (7: anything else is the default)
        got = on_device(ctx, coeffs, times, field, 0.01, 0.3, lanes=lanes)
        for name, a, b in zip(got._fields, got, base):
            assert np.array_equal(a, b, equal_nan=True), (lanes, name)
    near = m.DistanceField(grid, (0.0, 0.0, 0.0), 0.25, 0.1, "nearest")
    base = check_everything(ctx, coeffs, times, near, 0.01, 0.3)
    for lanes in (1, 64):
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(on_device(ctx, coeffs, times, near, 0.01, 0.3, lanes=lanes), base))


@pytest.mark.parametrize("lanes", [0, 1, 4, 16, 64])
def test_trajectory_atomics(ctx, lanes):
    """Among 70 clear trajectories of three segments (d = x, x >= 1): one whose only failing sample is the last sample of its last
    segment (x = 2 - t reaches 0 at T = 2), one that fails at the first sample of segment 0 (x = t), and one whose second
    segment has too many samples."""
    f = linear_field(0)
    coeffs = np.tile(line([2.0, 1.0, 0.5], [0.0, 0.0, 0.0]), (70, 3, 1, 1))          # [70][3][3][2]
    times = np.full((70, 3), 2.0)
    coeffs[17, 2, 0] = (2.0, -1.0)
    coeffs[66, 0, 0] = (0.0, 1.0)
    times[41, 1] = 9.0                                                               # S = 37 > 16
    d = on_device(ctx, coeffs, times, f, 0.25, max_samples=16, lanes=lanes)
    feas = np.ones(70, dtype=np.int32)
    feas[[17, 66, 41]] = 0
    fseg = np.full(70, -1, dtype=np.int32)
    fseg[[17, 66, 41]] = (2, 0, 1)
    assert np.array_equal(d.trajectory_feasible, feas) and np.array_equal(d.first_failing_segment, fseg)
    assert d.segment_first_failing_sample[17].tolist() == [-1, -1, 8] and d.segment_closest_sample[17].tolist() == [0, 0, 8]
    assert d.segment_first_failing_sample[66].tolist() == [0, -1, -1] and d.trajectory_clearance[[17, 66]].tolist() == [0.0, 0.0]
    assert d.segment_samples[41].tolist() == [9, -1, 9] and np.isnan(d.trajectory_clearance[41]) and np.isnan(d.segment_clearance[41, 1])
    assert d.first_failing_time[[17, 66]].tolist() == [2.0, 0.0] and np.isnan(d.first_failing_time[41])
    clear = feas == 1
    assert (d.trajectory_clearance[clear] == 2.0).all() and (d.segment_closest_sample[clear] == 0).all()
    import mav_trajectory_generation_amd as m
    h = m.check_distance_field_host(coeffs, times, f, 0.25, max_samples=16)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(d, h))


def test_optional_outputs_and_want_segments(ctx):
    import torch
    import mav_trajectory_generation_amd as m
    coeffs, times, grid, origin = field_case("n5_k3_d3")
    field = m.DistanceField(grid, origin, H, np.inf)
    full = on_device(ctx, coeffs, times, field, DT, INFLATION)
    bare = on_device(ctx, coeffs, times, field, DT, INFLATION, want_segments=False)
    assert bare.segment_clearance is None and bare.segment_samples is None and bare.segment_closest_time is None and bare.first_failing_time is None
    for name in ("trajectory_feasible", "first_failing_segment", "trajectory_clearance"):
        assert np.array_equal(getattr(bare, name), getattr(full, name)), name
    # only the verdict, in buffers with guard words
    co, ti, gr = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (coeffs, times, grid))
    bsz, k = times.shape
    feas = torch.full((bsz + 6,), -7, dtype=torch.int32, device="cuda")
    from mav_trajectory_generation_amd import _lib as L
    fc = L.DistanceFieldC(gr.data_ptr(), grid.shape[2], grid.shape[1], grid.shape[0], (ctypes.c_double * 3)(*origin), H, np.inf, 1)
    torch.cuda.synchronize()
    assert ctx.lib.mtg_check_distance_field(ctx.handle, 5, k, 3, bsz, co.data_ptr(), ti.data_ptr(), k, 1, ctypes.byref(fc), DT, 4096, INFLATION,
                                            feas.data_ptr() + 12, None, None, None, None, None, None) == 0
    ctx.sync()
    got = feas.cpu().numpy()
    assert (got[:3] == -7).all() and (got[-3:] == -7).all() and np.array_equal(got[3:-3], full.trajectory_feasible)


def test_capture_and_replay(ctx):
    """Three launches on the context's stream, a linear chain: captured once and replayed twice, the same bits as the direct call."""
    import torch
    import mav_trajectory_generation_amd as m
    from mav_trajectory_generation_amd import _lib as L
    coeffs, times, grid, origin = field_case("n10_k8_d3_fast")
    bsz, k = times.shape
    co, ti, gr = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (coeffs, times, grid))
    fc = L.DistanceFieldC(gr.data_ptr(), grid.shape[2], grid.shape[1], grid.shape[0], (ctypes.c_double * 3)(*origin), H, np.inf, 1)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    outs = [i32(bsz), i32(bsz), f64(bsz, k), i32(bsz, k), i32(bsz, k), i32(bsz, k), f64(bsz)]

    def call():
        assert ctx.lib.mtg_check_distance_field(ctx.handle, 10, k, 3, bsz, co.data_ptr(), ti.data_ptr(), k, 1, ctypes.byref(fc), DT, 4096,
                                                INFLATION, *[o.data_ptr() for o in outs]) == 0
    torch.cuda.synchronize()
    call()                                       # warm-up outside the capture (module load)
    ctx.sync()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(ctx.stream):
        with torch.cuda.graph(g, stream=ctx.stream):
            call()
    co.copy_(torch.flip(co, dims=(0,)))          # new values in the captured buffers
    ti.copy_(torch.flip(ti, dims=(0,)))
    torch.cuda.synchronize()
    want = on_device(ctx, coeffs[::-1], times[::-1], m.DistanceField(grid, origin, H, np.inf), DT, INFLATION)
    assert 0 < int(want.trajectory_feasible.sum()) < bsz
    for _ in range(2):
        for o in outs:
            o.fill_(-5)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for o, w in zip(outs, want[:7]):
            assert np.array_equal(o.cpu().numpy(), w, equal_nan=True)


def test_an_8_mib_grid_and_a_grid_two_voxels_wide(ctx):
    import mav_trajectory_generation_amd as m
    coeffs, times, _, _ = field_case("n12_k4_d4")
    rng = np.random.default_rng(128)
    big = R.spheres_field((-8.0, -8.0, -8.0), (128, 128, 128), 0.125, rng.uniform(-5.0, 5.0, (6, 3)), rng.uniform(0.3, 1.0, 6))
    assert big.nbytes == 8 << 20
    for interpolation in ("trilinear", "nearest"):
        d = check_everything(ctx, coeffs, times, m.DistanceField(big, (-8.0, -8.0, -8.0), 0.125, np.inf, interpolation), DT, INFLATION)
        assert 0 < d.trajectory_feasible.sum() < len(coeffs)
    # nx = 2: one cell across; a slab around the plane x = 0 in which the trajectories come and go
    thin = R.spheres_field((-0.125, -6.0, -6.0), (2, 49, 47), 0.25, [[0.0, 1.0, -1.0], [0.0, -3.0, 2.0]], [1.0, 0.7])
    for interpolation in ("trilinear", "nearest"):
        d = check_everything(ctx, coeffs, times, m.DistanceField(thin, (-0.125, -6.0, -6.0), 0.25, np.inf, interpolation), DT, INFLATION)
        inside = np.isfinite(d.segment_clearance)
        assert inside.any() and not inside.all()


def test_the_contexts_status_word_is_untouched(ctx):
    """A bad time that an EARLIER asynchronous solve left in the context's word is still reported by the next sync, after a check
    with failing trajectories in between; and the check itself leaves nothing there."""
    import mav_trajectory_generation_amd as m
    coeffs, times, grid, origin = field_case("n7_k4_d4")
    field = m.DistanceField(grid, origin, H)
    want = m.check_distance_field_host(coeffs, times, field, DT, inflation=INFLATION)
    d = on_device(ctx, coeffs, times, field, DT, INFLATION)          # (ends with ctx.sync(): it would raise)
    assert not d.trajectory_feasible.all() and np.array_equal(d.trajectory_feasible, want.trajectory_feasible)
    masks = m.ends_full_masks(10, 8)
    plan = m.Plan(ctx, 10, 3, 8, 4, masks)
    t, f = m.random_waypoint_batch(64, 8, 3, 10, masks, seed=2, device="cuda", layout="aos")
    t[5, 3] = -1.0
    plan.solve(t, f)                                                 # asynchronous: leaves BAD_TIME in the context's word
    with pytest.raises(m.MtgError) as e:
        on_device(ctx, coeffs, times, field, DT, INFLATION)
    assert e.value.code == -2
    ctx.sync()
    d = on_device(ctx, coeffs, times, field, DT, INFLATION)
    assert np.array_equal(d.first_failing_segment, want.first_failing_segment)
    plan.close()
