"""Per-axis extrema on the device (mtg_minmax_axes, csrc/mtg_axes.hip): against the reference's own Polynomial::computeMinMax
(tests/golden/reference_axis_minmax_*.npz), against the library's host build of the same lane code on the full fixtures and at
the shapes where the kernel could go wrong, and captured into a graph.  Values agree with the host form within the bound of
tests/axis_minmax_ref.py, not bit for bit: the device takes v_rcp_f64 in the Newton step."""
import numpy as np
import pytest

import axis_minmax_ref as ref
from test_axis_minmax import CASES, argument_table, load_case, numpy_fold

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import mav_trajectory_generation_amd as m
    c = m.Context(0)
    yield c
    c.close()


def on_device(ctx, coeffs, times, first, count, layout="aos", want_trajectory=True):
    import torch
    import mav_trajectory_generation_amd as m
    t = times if layout == "aos" else np.ascontiguousarray(times.T)
    out = m.minmax_axes(ctx, torch.from_numpy(np.ascontiguousarray(coeffs)).cuda(), torch.from_numpy(np.ascontiguousarray(t)).cuda(), first, count,
                        times_layout=layout, want_trajectory=want_trajectory)
    ctx.sync()
    return m.AxisMinMax(*[o.cpu().numpy() if o is not None else None for o in out])


def same_as_host(ctx, coeffs, times, first, count, layout="aos"):
    """Device against host form: values within the bound, every device row checked on its own, the device's reduction is the
    fold of the device's segment table.  Returns (device result, largest value difference / max(1, S))."""
    import mav_trajectory_generation_amd as m
    h = m.minmax_axes_host(coeffs, times, first, count)
    d = on_device(ctx, coeffs, times, first, count, layout)
    worst = ref.check_table(d.segment, coeffs, times, first, h.segment)
    traj, idx = numpy_fold(d.segment)
    assert np.array_equal(d.trajectory, traj) and np.array_equal(d.trajectory_segment_idx, idx)
    return d, worst


@pytest.mark.parametrize("name", CASES)
def test_device_entry_vs_reference(ctx, name):
    coeffs, times, want = load_case(name)
    orders = min(5, coeffs.shape[-1])
    d = on_device(ctx, coeffs, times, 0, orders)
    worst = ref.check_table(d.segment, coeffs, times, 0, want)
    print(f"{name}: device vs reference, worst |got - want| / max(1, S) = {worst:.2e}")
    d1 = on_device(ctx, coeffs, times, 1, min(2, orders - 1), want_trajectory=False)
    ref.check_table(d1.segment, coeffs, times, 1, want[:, :, :, 1:3])
    assert d1.trajectory is None


@pytest.mark.parametrize("name", CASES)
def test_device_vs_host_on_the_full_fixtures(ctx, name):
    """n10_k8_d3_fast whole: 2400 lanes = 37.5 workgroups."""
    coeffs, times, _ = load_case(name, whole=True)
    _, worst = same_as_host(ctx, coeffs, times, 0, min(5, coeffs.shape[-1]))
    print(f"{name}: device vs host, largest value difference / max(1, S) = {worst:.2e}")


@pytest.mark.parametrize("bsz,k,dim", [(1, 1, 1), (21, 1, 3), (8, 2, 4), (13, 5, 1), (43, 1, 3)])
def test_lane_counts_around_a_workgroup(ctx, bsz, k, dim):
    """1, 63, 64, 65 and 129 lanes."""
    assert bsz * k * dim in (1, 63, 64, 65, 129)
    coeffs, times = ref.family_sinusoid(np.random.default_rng(bsz), bsz, k, dim, 10)
    for layout in ("aos", "soa"):
        same_as_host(ctx, coeffs, times, 0, 5, layout)


def test_smallest_and_largest_instances(ctx):
    rng = np.random.default_rng(21)
    # N = 2: nothing searched; the extrema of a line are its ends
    coeffs, times = ref.family_taylor(rng, 5, 3, 3, 2)
    d, _ = same_as_host(ctx, coeffs, times, 0, 2)
    ends = np.stack([coeffs[..., 0], coeffs[..., 0] + coeffs[..., 1] * times[:, :, None]])
    assert np.abs(d.segment[..., 0, 1] - ends.min(axis=0)).max() <= 1e-14 and np.abs(d.segment[..., 0, 3] - ends.max(axis=0)).max() <= 1e-14
    assert np.array_equal(d.segment[..., 1, :], np.stack([0 * coeffs[..., 1], coeffs[..., 1], 0 * coeffs[..., 1], coeffs[..., 1]], axis=-1))
    # N = 3: a parabola c + b t + a t^2 with its vertex inside: the vertex value c - b^2 / (4 a)
    a, b, c = rng.uniform(0.5, 2.0, (7, 2, 3)), -rng.uniform(0.5, 2.0, (7, 2, 3)), rng.standard_normal((7, 2, 3))
    coeffs = np.stack([c, b, a], axis=-1)
    times = np.full((7, 2), 4.5)                        # vertex at -b / 2a in (0.125, 2)
    d, _ = same_as_host(ctx, coeffs, times, 0, 3)
    assert np.abs(d.segment[..., 0, 1] - (c - b * b / (4 * a))).max() <= 1e-12
    assert np.abs(d.segment[..., 0, 0] - (-b / (2 * a))).max() <= 1e-9
    # N = 12, first = 0, n = 5 with every critical point inside: M = 10, both root buffers full
    coeffs, times = ref.family_all_roots_inside(rng, 6, 2, 3, 12)
    want = ref.table(coeffs, times)
    d, _ = same_as_host(ctx, coeffs, times, 0, 5)
    ref.check_table(d.segment, coeffs, times, 0, want)
    # D = 8, and first = 4, n = 1
    coeffs, times = ref.family_taylor(rng, 3, 3, 8, 9)
    same_as_host(ctx, coeffs, times, 0, 5)
    d, _ = same_as_host(ctx, coeffs, times, 4, 1)
    ref.check_table(d.segment, coeffs, times, 4, ref.table(coeffs, times)[:, :, :, 4:5])


def test_guard_cells_null_outputs_nan_and_arguments(ctx):
    import torch
    import mav_trajectory_generation_amd as m
    coeffs, times = ref.family_sinusoid(np.random.default_rng(31), 9, 3, 3, 10)
    bsz, k, dim, n = coeffs.shape
    first, count, guard, fill = 1, 3, 16, -12345.678
    co, ti = torch.from_numpy(coeffs).cuda(), torch.from_numpy(times).cuda()
    seg = torch.full((guard + bsz * k * dim * count * 4 + guard,), fill, dtype=torch.float64, device="cuda")
    traj = torch.full((guard + bsz * dim * count * 4 + guard,), fill, dtype=torch.float64, device="cuda")
    idx = torch.full((guard + bsz * dim * count * 2 + guard,), -77, dtype=torch.int32, device="cuda")

    def call(n=n, k=k, d=dim, b=bsz, c=co.data_ptr(), t=ti.data_ptr(), sb=k, sk=1, first=first, count=count, seg=seg.data_ptr() + 8 * guard,
             traj=traj.data_ptr() + 8 * guard, idx=idx.data_ptr() + 4 * guard):
        return ctx.lib.mtg_minmax_axes(ctx.handle, n, k, d, b, c, t, sb, sk, first, count, seg, traj, idx)

    torch.cuda.synchronize()
    assert call(b=0) == 0                                 # batch = 0: nothing enqueued, nothing written
    assert call(seg=seg.data_ptr() + 8 * guard + 8) == -1  # 16-byte alignment
    assert b"aligned" in ctx.lib.mtg_last_error_string(ctx.handle)
    for bad in (dict(n=1), dict(n=13), dict(k=0), dict(d=0), dict(d=9), dict(b=-1), dict(sb=1, sk=1), dict(sb=0), dict(sk=-1),
                dict(first=-1), dict(first=5), dict(count=0), dict(count=6), dict(first=4, count=2), dict(n=4, first=3, count=2),
                dict(c=None), dict(t=None), dict(seg=None)):
        assert call(**bad) == -1, bad
    ctx.sync()
    assert (seg.cpu().numpy() == fill).all() and (traj.cpu().numpy() == fill).all() and (idx.cpu().numpy() == -77).all()
    assert call(traj=None, idx=None) == 0                 # NULL trajectory outputs
    ctx.sync()
    h = m.minmax_axes_host(coeffs, times, first, count)
    s1 = seg.cpu().numpy()
    assert (s1[:guard] == fill).all() and (s1[-guard:] == fill).all() and (s1[guard:-guard] != fill).all()
    assert (traj.cpu().numpy() == fill).all() and (idx.cpu().numpy() == -77).all()
    assert call() == 0
    ctx.sync()
    s2, t2, i2 = seg.cpu().numpy(), traj.cpu().numpy(), idx.cpu().numpy()
    assert np.array_equal(s1, s2)                         # the segment table does not depend on the trajectory outputs
    for a, f in ((s2, fill), (t2, fill), (i2, -77)):
        assert (a[:guard] == f).all() and (a[-guard:] == f).all() and (a[guard:-guard] != f).all()
    got = s2[guard:-guard].reshape(bsz, k, dim, count, 4)
    ref.check_table(got, coeffs, times, first, h.segment)
    want_traj, want_idx = numpy_fold(got)
    assert np.array_equal(t2[guard:-guard].reshape(bsz, dim, count, 4), want_traj)
    assert np.array_equal(i2[guard:-guard].reshape(bsz, dim, count, 2), want_idx)
    assert call(traj=traj.data_ptr() + 8 * guard, idx=None) == 0   # the trajectory table without the indices
    ctx.sync()
    assert np.array_equal(traj.cpu().numpy(), t2)
    # the NaN rule
    clean = on_device(ctx, coeffs, times, 0, 5)
    bad = coeffs.copy()
    bad[4, 1, 2, 2] = np.nan
    r = on_device(ctx, bad, times, 0, 5)
    nan_row = np.array([0.0, np.nan, 0.0, np.nan])
    for q in range(3):
        assert np.array_equal(r.segment[4, 1, 2, q], nan_row, equal_nan=True) and np.array_equal(r.trajectory[4, 2, q], nan_row, equal_nan=True)
        assert r.trajectory_segment_idx[4, 2, q].tolist() == [1, 1]
    mask = np.ones(r.segment.shape[:4], dtype=bool)
    mask[4, 1, 2, :3] = False
    assert np.array_equal(r.segment[mask], clean.segment[mask])


def test_capture_and_replay(ctx):
    """The call is a chain of two kernel launches on the context's stream: captured once, replayed on new coefficients."""
    import torch
    import mav_trajectory_generation_amd as m
    coeffs, times, _ = load_case("n10_k8_d3_fast", whole=True)
    bsz, k, dim, n = coeffs.shape
    co, ti = torch.from_numpy(np.ascontiguousarray(coeffs)).cuda(), torch.from_numpy(np.ascontiguousarray(times)).cuda()
    seg = torch.zeros((bsz, k, dim, 2, 4), dtype=torch.float64, device="cuda")
    traj = torch.zeros((bsz, dim, 2, 4), dtype=torch.float64, device="cuda")
    idx = torch.zeros((bsz, dim, 2, 2), dtype=torch.int32, device="cuda")

    def call():
        assert ctx.lib.mtg_minmax_axes(ctx.handle, n, k, dim, bsz, co.data_ptr(), ti.data_ptr(), k, 1, 1, 2, seg.data_ptr(), traj.data_ptr(),
                                       idx.data_ptr()) == 0
    torch.cuda.synchronize()
    call()                                       # warm-up outside the capture (module load)
    ctx.sync()
    first = seg.cpu().numpy().copy()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(ctx.stream):
        with torch.cuda.graph(g, stream=ctx.stream):
            call()
    co.copy_(torch.flip(co, dims=(0,)))          # new values in the captured buffers
    ti.copy_(torch.flip(ti, dims=(0,)))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(seg.cpu().numpy(), first[::-1])
    want_traj, want_idx = numpy_fold(first[::-1])
    assert np.array_equal(traj.cpu().numpy(), want_traj) and np.array_equal(idx.cpu().numpy(), want_idx)
    h = m.minmax_axes_host(coeffs[::-1], times[::-1], 1, 2)
    ref.check_table(seg.cpu().numpy(), np.ascontiguousarray(coeffs[::-1]), np.ascontiguousarray(times[::-1]), 1, h.segment)


def test_bounding_boxes(ctx):
    import torch
    import mav_trajectory_generation_amd as m
    coeffs, times, _ = load_case("n12_k4_d4", whole=True)
    co, ti = torch.from_numpy(np.ascontiguousarray(coeffs)).cuda(), torch.from_numpy(np.ascontiguousarray(times)).cuda()
    r = m.minmax_axes(ctx, co, ti, 0, 1)
    seg, traj = m.bounding_boxes(ctx, co, ti, margin=0.25)
    ctx.sync()
    bsz, k, dim, _ = coeffs.shape
    assert tuple(seg.shape) == (bsz, k, 2, dim) and tuple(traj.shape) == (bsz, 2, dim)
    s, t = r.segment.cpu().numpy(), r.trajectory.cpu().numpy()
    assert np.array_equal(seg.cpu().numpy()[:, :, 0], s[:, :, :, 0, 1] - 0.25) and np.array_equal(seg.cpu().numpy()[:, :, 1], s[:, :, :, 0, 3] + 0.25)
    assert np.array_equal(traj.cpu().numpy()[:, 0], t[:, :, 0, 1] - 0.25) and np.array_equal(traj.cpu().numpy()[:, 1], t[:, :, 0, 3] + 0.25)
    assert np.array_equal(traj.cpu().numpy()[:, 0], seg.cpu().numpy()[:, :, 0].min(axis=1))
    assert np.array_equal(traj.cpu().numpy()[:, 1], seg.cpu().numpy()[:, :, 1].max(axis=1))
    soa, _ = m.bounding_boxes(ctx, co, ti.t().contiguous(), times_layout="soa", margin=0.25)
    ctx.sync()
    assert np.array_equal(soa.cpu().numpy(), seg.cpu().numpy())
