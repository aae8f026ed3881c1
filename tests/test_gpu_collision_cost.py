"""Distance-field collision cost and gradient on the device (mtg_collision_cost): every instantiation with and without the
gradient, the sample counts around the lane partition, the rule's degenerate segments, guard words, both times layouts, against
the longdouble reference and against the host form; one fixture end to end."""
import ctypes

import numpy as np
import pytest

import collision_cost_ref as C
from test_collision_cost import EPSILON, SPEED_EPSILON, compare
from test_distance_field import DT, H, INFLATION, field_case

pytestmark = pytest.mark.gpu
B, K = 3, 3
NX, NY, NZ = 9, 8, 7
VOXEL, ORIGIN, OUTSIDE = 0.25, (-0.5, 0.25, 1.0), 0.125
LENGTHS = (2, 3, 63, 64, 65, 129)     # S of the six plain segments; the others: T = 0, NaN T, S > max_samples
MAX_SAMPLES = 140
GUARD = 4


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import mav_trajectory_generation_amd as m
    c = m.Context(0)
    yield c
    c.close()


def grid_9_8_7():
    rng = np.random.default_rng(987)
    return rng.uniform(-0.2, 1.0, (NZ, NY, NX)).astype(np.float32)


def case(n, d):
    """(coeffs [3][3][d][n], times [3][3], dt, special [3][3]): paths through and around the grid."""
    rng = np.random.default_rng(100 * n + d)
    dt = 0.02 + 0.001 * n
    T = np.array([(S - 2 + 0.5) * dt for S in LENGTHS] + [0.0, np.nan, (MAX_SAMPLES + 10) * dt])
    T = T[rng.permutation(9)].reshape(B, K)
    lo = np.array(ORIGIN)
    hi = lo + VOXEL * (np.array([NX, NY, NZ]) - 1)
    coeffs = rng.normal(size=(B, K, d, n))                      # (the yaw row stays noise: it is never read)
    for b in range(B):
        for k in range(K):
            scale = T[b, k] if T[b, k] > 0 else 1.0
            start, end = rng.uniform(lo - 0.1, hi + 0.1), rng.uniform(lo - 0.1, hi + 0.1)
            coeffs[b, k, :3, 0] = start
            for i in range(1, n):
                a = (end - start) if i == 1 else rng.normal(size=3) * 0.3 / i
                coeffs[b, k, :3, i] = a / scale ** i
    special = ~(T > 0) | (T > MAX_SAMPLES * dt)
    return coeffs, T, dt, special


def raw_device_call(ctx, coeffs, times, grid, dt, layout="aos", gradient=True):
    """mtg_collision_cost into NaN-filled buffers between guard words; the four outputs as numpy arrays."""
    import torch
    from mav_trajectory_generation_amd import _lib as L
    b, k, d, n = coeffs.shape
    t = times if layout == "aos" else np.ascontiguousarray(times.T)
    strides = (k, 1) if layout == "aos" else (1, b)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    c_d, t_d, g_d = dev(coeffs), dev(t), dev(grid)
    field = L.DistanceFieldC(g_d.data_ptr(), NX, NY, NZ, (ctypes.c_double * 3)(*ORIGIN), VOXEL, OUTSIDE, 1)

    def guarded(count, dtype, fill):
        buf = torch.full((count + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        buf[:GUARD] = -77
        buf[-GUARD:] = -77
        return buf
    seg, traj = guarded(b * k, torch.float64, float("nan")), guarded(b, torch.float64, float("nan"))
    grad, smp = guarded(b * k * d * n, torch.float64, float("nan")), guarded(b * k, torch.int32, -5)
    ptr = lambda buf: buf.data_ptr() + GUARD * buf.element_size()
    cur = ctx._enter()
    try:
        rc = ctx.lib.mtg_collision_cost(ctx.handle, n, k, d, b, c_d.data_ptr(), t_d.data_ptr(), *strides, ctypes.byref(field), dt, MAX_SAMPLES,
                                        INFLATION, EPSILON, SPEED_EPSILON, ptr(seg), ptr(traj), ptr(grad) if gradient else None, ptr(smp))
    finally:
        ctx._leave(cur)
    assert rc == 0
    ctx.sync()
    out = []
    for buf in (traj, seg, grad, smp):
        a = buf.cpu().numpy()
        assert (a[:GUARD] == -77).all() and (a[-GUARD:] == -77).all()
        out.append(a[GUARD:-GUARD])
    import mav_trajectory_generation_amd as m
    if not gradient:
        assert np.isnan(out[2]).all()      # untouched
    return m.CollisionCostResult(out[0], out[1].reshape(b, k), out[2].reshape(b, k, d, n) if gradient else None, out[3].reshape(b, k))


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("d", [3, 4])
@pytest.mark.parametrize("n", [1, 4, 5, 7, 8, 10, 12])
def test_every_instantiation_against_the_reference_and_the_host(ctx, n, d):
    import mav_trajectory_generation_amd as m
    coeffs, T, dt, special = case(n, d)
    grid = grid_9_8_7()
    ref = C.reference(coeffs, T, grid, ORIGIN, VOXEL, OUTSIDE, dt, INFLATION, EPSILON, SPEED_EPSILON)
    assert sorted(ref["S"][~special]) == sorted(LENGTHS) and (ref["abs_cost"][~special] > 0).any()
    h = m.collision_cost_host(coeffs, T, m.DistanceField(grid, ORIGIN, VOXEL, OUTSIDE), dt, inflation=INFLATION, epsilon=EPSILON,
                              speed_epsilon=SPEED_EPSILON, max_samples=MAX_SAMPLES)
    r = raw_device_call(ctx, coeffs, T, grid, dt)
    # the rule's own values
    assert np.array_equal(r.segment_samples, h.segment_samples)
    zero, nan, capped = T == 0.0, np.isnan(T), T > MAX_SAMPLES * dt
    assert list(r.segment_samples[zero]) == [2] and list(r.segment_samples[nan]) == [2] and list(r.segment_samples[capped]) == [-1]
    assert r.segment_cost[zero][0] == 0.0 and (r.coeff_gradient[zero] == 0.0).all()
    for which in (nan, capped):
        assert np.isnan(r.segment_cost[which]).all() and np.isnan(r.coeff_gradient[which][:, :3]).all()
    assert (r.coeff_gradient[:, :, 3:] == 0.0).all()
    total = np.zeros(B)
    for k in range(K):
        total = total + r.segment_cost[:, k]
    assert same(r.trajectory_cost, total)
    # every float output within the reference's bound; the device and the host within the sum of the two bounds
    share = compare(ref, r, f"device n{n} d{d}", special=special)
    ok = ~special & ~ref["fragile"].any(axis=2)
    assert (np.abs(r.segment_cost - h.segment_cost)[ok] <= 2.0 * ref["bound_cost"][ok]).all()
    assert (np.abs(r.coeff_gradient - h.coeff_gradient)[:, :, :3][ok] <= 2.0 * ref["bound_grad"][ok]).all()
    bitwise = all(same(x, y) for x, y in zip(r, h))
    print(f"n{n} d{d}: largest share of the bound on the device {share:.3e}; device == host bit for bit: {bitwise}")
    # the other layout and the cost-only instantiation
    soa = raw_device_call(ctx, coeffs, T, grid, dt, layout="soa")
    assert all(same(x, y) for x, y in zip(r, soa))
    cost_only = raw_device_call(ctx, coeffs, T, grid, dt, gradient=False)
    assert same(cost_only.segment_cost, r.segment_cost) and same(cost_only.trajectory_cost, r.trajectory_cost)
    assert np.array_equal(cost_only.segment_samples, r.segment_samples)


def test_a_fixture_end_to_end(ctx):
    import torch
    import mav_trajectory_generation_amd as m
    coeffs, times, grid, origin = field_case("n10_k8_d3_fast")
    kw = dict(inflation=INFLATION, epsilon=EPSILON, speed_epsilon=SPEED_EPSILON)
    h = m.collision_cost_host(coeffs, times, m.DistanceField(grid, origin, H, 0.0), DT, **kw)
    dev = m.DistanceField(torch.from_numpy(grid).cuda(), origin, H, 0.0)
    c_d, t_d = torch.from_numpy(coeffs).cuda(), torch.from_numpy(times).cuda()
    r = m.collision_cost(ctx, c_d, t_d, dev, DT, **kw)
    r0 = m.collision_cost(ctx, c_d, t_d, dev, DT, want_gradient=False, **kw)
    ctx.sync()
    r = m.CollisionCostResult(*[x.cpu().numpy() for x in r])
    assert r0.coeff_gradient is None and same(r0.segment_cost.cpu().numpy(), r.segment_cost)
    assert same(r0.trajectory_cost.cpu().numpy(), r.trajectory_cost)
    ref = C.reference(coeffs, times, grid, origin, H, 0.0, DT, INFLATION, EPSILON, SPEED_EPSILON)
    share = compare(ref, r, "device n10_k8_d3_fast")
    ok = ~ref["fragile"].any(axis=2)
    assert np.array_equal(r.segment_samples, h.segment_samples)
    assert (np.abs(r.segment_cost - h.segment_cost)[ok] <= 2.0 * ref["bound_cost"][ok]).all()
    assert (np.abs(r.coeff_gradient - h.coeff_gradient)[ok] <= 2.0 * ref["bound_grad"][ok]).all()
    assert (np.abs(r.trajectory_cost - h.trajectory_cost) <= 2.0 * ref["bound_cost"].sum(axis=1) + 8 * C.EPS * np.abs(h.trajectory_cost)).all()
    print(f"fixture: largest share of the bound on the device {share:.3e}; device == host bit for bit: "
          f"{all(same(x, y) for x, y in zip(r, h))}")
