"""Every device instantiation of the time objective's maxima search: mtg_objective_seg_kernel<NC, DC>, NC in {4, 6, 8, 10, 12} x
DC in {3, 4}, through mtg_magnitude_soft_cost on the inputs, the reference and the bounds of tests/test_objective_instances.py
(N = 4 .. 12 at D = 3 and 4, D = 1 and 2 at N = 10 and 7, every order 1 .. N/2 - 1, all three input families; 13 trajectories x 5
segments = one full workgroup and one lane), against the host form, with both time layouts; the zero-padded paths, the
constraint-list forms and non-finite coefficients on the device; mtg_time_objective through a plan at N = 6 and N = 8.

Every device call of mtg_magnitude_soft_cost here writes into buffers filled with a marked NaN and followed by 64 guard words:
no guard may change and every output element must be written."""
import ctypes

import numpy as np
import pytest

import objective_ref as R
import test_objective_instances as H

pytestmark = pytest.mark.gpu
GUARD = 64
FILL_BITS = 0x7FF8DEAD0000BEEF      # a NaN no computation produces: "not written" is a comparison of bit patterns


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import mav_trajectory_generation_amd as m
    c = m.Context(0)
    yield c
    c.close()


def guarded_buffer(numel):
    import torch
    return torch.full((numel + GUARD,), FILL_BITS, dtype=torch.int64, device="cuda")


def device_fn(ctx):
    """mtg_magnitude_soft_cost with the signature of magnitude_soft_cost_host (numpy in, numpy out), guarded."""
    import torch
    import mav_trajectory_generation_amd as m

    def fn(coeffs, times, p, times_layout="aos"):
        co = torch.from_numpy(np.array(coeffs, dtype=np.float64, order="C")).cuda()      # (a copy: the shared inputs are read-only)
        tt = torch.from_numpy(np.array(times, dtype=np.float64, order="C")).cuda()
        bsz, k, dim, n = co.shape
        nc = p.n_constraints
        bufs = [guarded_buffer(bsz), guarded_buffer(bsz * nc), guarded_buffer(bsz * nc)]
        sb, sk = (k, 1) if times_layout == "aos" else (1, bsz)
        c = p.to_c()
        cur = ctx._enter()
        rc = ctx.lib.mtg_magnitude_soft_cost(ctx.handle, n, k, dim, bsz, ctypes.c_void_p(co.data_ptr()), ctypes.c_void_p(tt.data_ptr()),
                                             sb, sk, ctypes.byref(c), ctypes.c_void_p(bufs[0].data_ptr()),
                                             ctypes.c_void_p(bufs[1].data_ptr()) if nc else None,
                                             ctypes.c_void_p(bufs[2].data_ptr()) if nc else None)
        ctx._leave(cur)
        m.core._check(ctx.lib, rc, ctx.handle)
        ctx.sync()
        out = []
        for buf, numel in zip(bufs, (bsz, bsz * nc, bsz * nc)):
            host = buf.cpu().numpy()
            assert (host[numel:] == np.int64(FILL_BITS)).all(), "a guard word changed"
            assert (host[:numel] != np.int64(FILL_BITS)).all(), "an output element was not written"
            out.append(host[:numel].view(np.float64).copy())
        return out[0], out[1].reshape(bsz, nc), out[2].reshape(bsz, nc)
    return fn


def test_matrix_reaches_every_instantiation():
    """The launch list of test_device_matrix: the dispatch of mtg_objective.hip (N rounded up to even, D up to 3) sends its
    shapes to all ten mtg_objective_seg_kernel<NC, DC>."""
    reached = {((n + 1) & ~1, max(d, 3)) for n, d in R.SHAPES}
    assert reached == {(nc, dc) for nc in (4, 6, 8, 10, 12) for dc in (3, 4)}


WORST = {}


@pytest.mark.parametrize("n,d,family", R.CASES, ids=H.CASE_IDS)
def test_device_matrix(ctx, n, d, family):
    import mav_trajectory_generation_amd as m
    fn = device_fn(ctx)
    z = R.reference(n, d, family)
    costs, maxima, violations = H.run_groups(fn, n, z["coeffs"], z["times"], z["limits"])
    short, excess = H.check_bounds(maxima, z, n, d, f"device {family} n = {n} d = {d}")
    s2, e2 = H.check_segments(fn, z, n, d, maxima, f"device {family} n = {n} d = {d}")
    short, excess = max(short, s2), max(excess, e2)
    w = WORST.setdefault(n, [-np.inf, -np.inf])
    w[0], w[1] = max(w[0], short), max(w[1], excess)
    print(f"device, N = {n} so far: worst shortfall {w[0]:.3e}, worst excess {w[1]:.3e}")
    assert np.array_equal(violations, maxima - z["limits"])
    # against the host form: the figure of test_soft_cost_device_vs_host
    h_costs, h_max, h_vio = H.run_groups(m.magnitude_soft_cost_host, n, z["coeffs"], z["times"], z["limits"])
    rel = np.abs(maxima - h_max) / h_max
    print(f"device vs host {family} n = {n} d = {d}: worst relative difference of a maximum {rel.max():.2e}")
    allowed = 1e-12 * h_max
    if family == "allreal":
        # (both are evaluations of the magnitude at the maximiser as each side located it -- 1 / x in a Newton step is
        # v_rcp_f64 on the device -- and at up to eleven roots inside the segment the evaluation itself is good to the derived
        # bound only, up to 8e-10 at N = 10: each side may be off by that much, in either direction)
        allowed = allowed + 2.0 * (R.upper_bound_segments(z, n, d).max(axis=1) - z["traj"]).astype(np.float64)
    assert (np.abs(maxima - h_max) <= allowed).all()
    # each soft term on its own, from the device's maximum
    for q, der in enumerate(z["orders"]):
        c1, m1, v1 = fn(z["coeffs"], z["times"], H.params([(der, float(z["limits"][q]))]))
        assert np.array_equal(m1[:, 0], maxima[:, q]) and np.array_equal(v1[:, 0], violations[:, q])
        H.check_terms(c1, maxima[:, q], z["limits"][q], f"device n = {n} d = {d} order {der}")
    # [K][B] times: bit-equal
    for group, cost in zip(R.order_groups(n), costs):
        p = H.params([(der, float(z["limits"][der - 1])) for der in group])
        c2, m2, v2 = fn(z["coeffs"], np.ascontiguousarray(z["times"].T), p, times_layout="soa")
        assert np.array_equal(c2, cost) and np.array_equal(m2, maxima[:, group[0] - 1:group[-1]])
        assert np.array_equal(v2, violations[:, group[0] - 1:group[-1]])


@pytest.mark.parametrize("n,d,family", H.PADDING_CASES, ids=H.PADDING_IDS)
def test_zero_padding_device(ctx, n, d, family):
    H.check_padding(device_fn(ctx), n, d, family, np.array_equal)


@pytest.mark.parametrize("n,d", [(8, 3), (9, 4), (12, 4)])
def test_constraint_list_forms_device(ctx, n, d):
    H.check_constraint_list(device_fn(ctx), n, d)


def test_order_acceptance_device(ctx):
    H.check_order_acceptance(device_fn(ctx))


@pytest.mark.parametrize("n,d", H.NONFINITE_SHAPES)
def test_non_finite_device(ctx, n, d):
    """The host form first; then the device: NaN at the same positions, every finite trajectory bit-equal to the clean device run
    (check_non_finite), the poisoned trajectory's neighbours in the wavefront and the one across the workgroup boundary included."""
    import mav_trajectory_generation_amd as m
    host = H.check_non_finite(m.magnitude_soft_cost_host, n, d)
    dev = H.check_non_finite(device_fn(ctx), n, d)
    for group in host:
        for h, g in zip(host[group], dev[group]):
            assert np.array_equal(np.isnan(h), np.isnan(g))
        bad = np.isnan(host[group][1]).any(axis=1)
        assert np.array_equal(host[group][0][bad], dev[group][0][bad])      # maximum_cost per constraint, exactly, on both


@pytest.mark.parametrize("n", [6, 8])
def test_time_objective_through_a_plan(ctx, n):
    """mtg_time_objective at N = 6 and 8 (<6,3> and <8,3> by the plan route): coefficients of the plan's solve, maxima of
    mtg_magnitude_soft_cost on them, the total the left-to-right sum of its components, cost_time of mtg_time_cost_host."""
    import torch
    import mav_trajectory_generation_amd as m
    dim, k, bsz = 3, R.K, R.B
    plan = m.Plan(ctx, n, dim, k, n // 2 - 1, m.ends_full_masks(n, k, 1))
    times, d_fixed = plan.generate_waypoints(bsz, seed=606 + n, layout="aos")
    cons = [(der, 2.0 + der) for der in R.orders_of(n)]
    p = H.params(cons)
    res = m.time_objective(plan, times, d_fixed, p)
    status = torch.zeros((bsz,), dtype=torch.int32, device="cuda")
    coeffs, _, cost = plan.solve(times, d_fixed, want_cost=True, traj_status=status)
    ctx.sync()
    assert (status.cpu().numpy() == 0).all()
    assert np.array_equal(res.coeffs.cpu().numpy(), coeffs.cpu().numpy())
    comp, total = res.components.cpu().numpy(), res.objective.cpu().numpy()
    # (the solve adds the dimensions' cost shares with atomicAdd: three non-negative summands in arrival order, each order
    # within 2 eps of the exact sum)
    assert (np.abs(comp[:, 0] - cost.cpu().numpy()) <= 4 * H.EPS * comp[:, 0]).all()
    soft, maxima, violations = device_fn(ctx)(coeffs.cpu().numpy(), times.cpu().numpy(), p)
    assert np.isfinite(maxima).all() and (maxima > 0).all()
    assert np.array_equal(res.maxima.cpu().numpy(), maxima) and np.array_equal(res.violations.cpu().numpy(), violations)
    assert np.array_equal(comp[:, 2], soft)
    assert np.array_equal(total, (comp[:, 0] + comp[:, 1]) + comp[:, 2])
    assert np.array_equal(comp[:, 1], m.time_cost_host(times.cpu().numpy(), p))
    plan.close()
