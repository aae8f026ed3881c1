"""Nonlinear time objective with soft constraints on the device: mtg_time_objective against the reference's own callback values
(tests/golden/reference_time_objective_*.npz), mtg_magnitude_soft_cost against the library's host build of the same lane code,
the pattern search on top of them, and bad input.  Comparison rules: tests/time_objective_checks.py; the tolerances are the
coefficient parity tol_for(n, d) of tests/test_gpu_vs_reference.py (restated), twice that for a maximum (coefficient parity plus
extrema parity), and what follows from those for the soft terms and the total."""
import numpy as np
import pytest

import helpers
import time_objective_checks as C
from mav_trajectory_generation_amd import time_objective, magnitude_soft_cost, pattern_search_segment_times  # noqa: F401  (the feature under test)

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def tol_for(n, d):
    if n == 12 and d < n // 2 - 1:
        return 1e-5
    if n == 12 or d < n // 2 - 1:
        return 5e-8
    return 1e-9


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import mav_trajectory_generation_amd as m
    c = m.Context(0)
    yield c
    c.close()


def to_device(a, layout, kind):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if layout == "soa":
        t = t.t().contiguous() if kind == "times" else t.permute(1, 2, 0).contiguous()
    return t


def check_against(z, res, ctx, label):
    """The rule of the issue's check 4 on one result: z holds the reference values (a fixture, or an oracle evaluation)."""
    import mav_trajectory_generation_amd as m
    n, d = int(z["n"]), int(z["d"])
    tol = tol_for(n, d)
    comp, total = res.components.cpu().numpy(), res.objective.cpu().numpy()
    maxima, violations = res.maxima.cpu().numpy(), res.violations.cpu().numpy()
    ref = z["components"]
    rel = np.abs(comp[:, 0] - ref[:, 0]) / ref[:, 0]
    print(f"{label}: cost_trajectory worst relative difference {rel.max():.2e} (allowed {tol:.0e}); "
          f"cost_time {np.abs(comp[:, 1] / ref[:, 1] - 1).max():.2e}")
    assert (rel <= tol).all()
    assert (np.abs(comp[:, 1] - ref[:, 1]) <= 1e-14 * ref[:, 1]).all()
    C.check_maxima(maxima, z, 2 * tol, extra_up=tol, label=label)
    assert np.array_equal(violations, maxima - z["con_value"])
    if int(z["use_soft_constraints"]):
        t_dev = to_device(z["times"], "aos", "times")
        for q in range(len(z["con_value"])):      # each term on its own: the soft cost of constraint q alone on the SAME coefficients
            term, mx, _ = m.magnitude_soft_cost(ctx, res.coeffs, t_dev, C.params_of(z, only=q))
            ctx.sync()
            assert np.array_equal(mx.cpu().numpy()[:, 0], maxima[:, q])
            C.check_term(term.cpu().numpy(), z, q, 2 * tol, extra_up=tol, label=label)
        ref_sum, below, above = C.soft_sum_bounds(z, 2 * tol, extra_up=tol)
        slack = 8 * EPS * ref_sum
        assert (comp[:, 2] >= ref_sum - below - slack).all() and (comp[:, 2] <= ref_sum + above + slack).all()
    else:
        ref_sum = below = above = np.zeros(len(total))
        assert (comp[:, 2] == 0.0).all()
    # the total: within the sum of the component bounds (plus the rounding of two additions)
    ref_total = z["total"]
    lo = tol * ref[:, 0] + 1e-14 * ref[:, 1] + below + 8 * EPS * np.abs(ref_total)
    hi = tol * ref[:, 0] + 1e-14 * ref[:, 1] + above + 8 * EPS * np.abs(ref_total)
    assert (total >= ref_total - lo).all() and (total <= ref_total + hi).all()
    assert np.array_equal(total, comp[:, 0] + comp[:, 1] + comp[:, 2])


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_time_objective_vs_reference(ctx, name, layout):
    """Check 4: every fixture, both layouts; the free-constraint form where the fixture has d_free."""
    import mav_trajectory_generation_amd as m
    z = C.load(name)
    n, d = int(z["n"]), int(z["d"])
    masks = [int(v) for v in z["masks"]]
    bsz, k = z["times"].shape
    dim = z["d_fixed"].shape[1]
    assert C.near_cap(z, 2 * tol_for(n, d), tol_for(n, d)).mean() <= 0.0
    plan = m.Plan(ctx, n, dim, k, d, masks)
    d_free = to_device(z["d_free"], layout, "fixed") if "d_free" in z.files else None
    res = m.time_objective(plan, to_device(z["times"], layout, "times"), to_device(z["d_fixed"], layout, "fixed"), C.params_of(z),
                           d_free=d_free, layout=layout)
    ctx.sync()
    assert helpers.poly_relerr(res.coeffs.cpu().numpy(), z["coeffs_ref"]) < tol_for(n, d)
    check_against(z, res, ctx, f"{name}/{layout}")
    plan.close()


@pytest.mark.parametrize("n,d,k,dim,interior,bsz", [(10, 4, 8, 3, 1, 10000), (10, 4, 16, 4, 7, 12500)])
def test_soft_cost_device_vs_host(ctx, n, d, k, dim, interior, bsz):
    """Check 5: the device search against the host build of the same lane code on solved coefficients, maxima within 1e-12."""
    import mav_trajectory_generation_amd as m
    masks = m.ends_full_masks(n, k, interior)
    plan = m.Plan(ctx, n, dim, k, d, masks)
    times, d_fixed = plan.generate_waypoints(bsz, seed=77, layout="aos", yaw_dim=(dim == 4))
    coeffs, _, _ = plan.solve(times, d_fixed)
    p = m.TimeObjectiveParams(constraints=[(1, 3.0), (2, 5.0)])
    cost, maxima, violations = m.magnitude_soft_cost(ctx, coeffs, times, p)
    ctx.sync()
    h_cost, h_max, h_vio = m.magnitude_soft_cost_host(coeffs.cpu().numpy(), times.cpu().numpy(), p)
    rel = np.abs(maxima.cpu().numpy() - h_max) / h_max
    print(f"{bsz} x {k}: worst relative difference of a maximum, device vs host: {rel.max():.2e}")
    assert (rel <= 1e-12).all()
    assert (np.abs(violations.cpu().numpy() - h_vio) <= 1e-12 * h_max).all()
    # the same maxima give the same terms up to exp's last bits and the exponent's sensitivity to the 1e-12
    got, capped = cost.cpu().numpy(), h_cost >= 1e12
    assert np.array_equal(got[capped] >= 1e12, h_cost[capped] >= 1e12)
    band = 100.0 * (h_max / np.array([3.0, 5.0])).max(axis=1) * 1e-12 + 1e-13
    both = (got < 1e12) & (h_cost < 1e12)
    assert (np.abs(got[both] - h_cost[both]) <= h_cost[both] * np.expm1(band[both])).all()
    # times in the other layout: the same answer
    cost2, maxima2, _ = m.magnitude_soft_cost(ctx, coeffs, times.t().contiguous(), p, times_layout="soa")
    ctx.sync()
    assert np.array_equal(maxima2.cpu().numpy(), maxima.cpu().numpy()) and np.array_equal(cost2.cpu().numpy(), got)
    plan.close()


def oracle_reference(z, times, rows):
    """The objective of trajectories `rows` at `times` from oracle_np + oracle_extrema, shaped like a fixture."""
    from oracle import oracle_np as onp
    from oracle import oracle_extrema as ox
    masks = [int(v) for v in z["masks"]]
    n, d = int(z["n"]), int(z["d"])
    co, _, cost = onp.solve_batch(n, d, masks, times[rows], z["d_fixed"][rows])
    maxima = np.array([[ox.trajectory_min_max_magnitude(co[i], times[b], int(der))[1][1] for der in z["con_derivative"]]
                       for i, b in enumerate(rows)])
    out = {key: z[key] for key in ("n", "d", "con_derivative", "con_value", "soft_constraint_weight", "maximum_cost", "use_soft_constraints",
                                   "time_cost_kind", "time_penalty")}
    out["times"], out["maxima"] = times[rows], maxima
    total_time = np.array([sum(times[b].tolist()) for b in rows])
    cost_time = total_time * total_time * float(z["time_penalty"])
    terms, _ = C.reference_terms(out)
    out["components"] = np.stack([cost, cost_time, terms.sum(axis=1)], axis=1)
    out["total"] = out["components"].sum(axis=1)
    return out


def test_pattern_search(ctx):
    """Check 6, on the `search` fixture."""
    import torch
    import mav_trajectory_generation_amd as m
    z = np.load(C.SEARCH)
    n, d = int(z["n"]), int(z["d"])
    masks = [int(v) for v in z["masks"]]
    bsz, k = z["times"].shape
    p = C.params_of(z)
    plan = m.Plan(ctx, n, 3, k, d, masks)
    t0, f = to_device(z["times"], "aos", "times"), to_device(z["d_fixed"], "aos", "fixed")
    n_it, step0, lower = int(z["n_iterations"]), float(z["step0"]), float(z["lower_bound"])
    res = m.pattern_search_segment_times(plan, t0, f, p, n_iterations=n_it, step0=step0, lower_bound=lower)
    ctx.sync()
    history, final, times = res.history.cpu().numpy(), res.objective.cpu().numpy(), res.times.cpu().numpy()
    assert history.shape == (n_it + 1, bsz) and np.isfinite(history).all()
    assert (np.diff(history, axis=0) <= 0.0).all()                                   # non-increasing for every trajectory
    fresh = m.time_objective(plan, res.times, f, p)
    ctx.sync()
    assert np.array_equal(fresh.objective.cpu().numpy(), final)                      # bit for bit
    assert np.array_equal(fresh.coeffs.cpu().numpy(), res.coeffs.cpu().numpy())
    rows = [0, 9, 18, 31]
    zo = oracle_reference(z, times, rows)
    assert C.near_cap(zo, 2 * tol_for(n, d), tol_for(n, d)).mean() <= 0.0
    sub = m.time_objective(plan, res.times[rows].contiguous(), f[rows].contiguous(), p)
    ctx.sync()
    check_against(zo, sub, ctx, "search result vs oracle")
    # before its first accepted step the loop evaluates the reference loop's candidates: iteration 0 for every trajectory, and
    # every later iteration up to a trajectory's first accepted one, from the initial times and the halved steps
    ref_cand, first = z["candidates_objective"], z["first_accept_iteration"]
    for it in range(n_it):
        rows_it = np.nonzero((first < 0) | (first >= it))[0]
        if rows_it.size == 0:
            break
        step = step0 * 0.5 ** it
        cand = np.stack([z["times"][rows_it]] * (2 * k + 1))                         # [2K + 1][rows][K]
        for j in range(k):
            cand[1 + j, :, j] = z["times"][rows_it, j] * (1.0 + step)
            cand[1 + k + j, :, j] = np.maximum(lower, z["times"][rows_it, j] * (1.0 - step))
        flat = torch.from_numpy(cand.reshape(-1, k)).cuda()
        f_rep = f[torch.from_numpy(np.tile(rows_it, 2 * k + 1)).cuda()].contiguous()
        got = m.time_objective(plan, flat, f_rep, p).objective.cpu().numpy().reshape(2 * k + 1, -1)
        ref = ref_cand[it][:, rows_it]
        rel = np.abs(got - ref) / np.abs(ref)
        print(f"iteration {it}: {rows_it.size} trajectories before their first accepted step, candidates within {rel.max():.2e}")
        assert (rel <= 1e-7).all()
    ctx.sync()
    improved = z["first_accept_improvement"] > 1e-6
    assert improved.sum() >= 8 and (final[improved] < history[0][improved]).all()    # strictly below the initial
    assert (np.abs(history[0] - z["initial"]) <= 1e-7 * z["initial"]).all()
    print("final objective, ours / reference's loop (not asserted: paths may part at near-ties):")
    for b in range(bsz):
        print(f"  {b:2d}: initial {history[0][b]:.6e}  ours {final[b]:.6e}  reference {z['final_objective'][b]:.6e}")
    plan.close()


def test_bad_segment_time(ctx):
    """Check 7: a non-positive segment time gives +inf for that trajectory only, and the flag at sync."""
    import mav_trajectory_generation_amd as m
    z = C.load("n10_k8_d3_squared")
    masks = [int(v) for v in z["masks"]]
    plan = m.Plan(ctx, 10, 3, 8, 4, masks)
    times = z["times"][:16].copy()
    times[5, 3] = -1.0
    times[11, 0] = 0.0
    res = m.time_objective(plan, to_device(times, "aos", "times"), to_device(z["d_fixed"][:16], "aos", "fixed"), C.params_of(z))
    with pytest.raises(m.MtgError) as e:
        ctx.sync()
    assert e.value.code == -2
    total = res.objective.cpu().numpy()
    good = np.ones(16, dtype=bool)
    good[[5, 11]] = False
    assert np.isposinf(total[~good]).all() and np.isfinite(total[good]).all()
    # ... for that trajectory only: the others are what the same call gives them without the bad rows
    clean = m.time_objective(plan, to_device(z["times"][:16], "aos", "times"), to_device(z["d_fixed"][:16], "aos", "fixed"), C.params_of(z))
    ctx.sync()
    assert np.array_equal(total[good], clean.objective.cpu().numpy()[good])
    assert np.array_equal(res.components.cpu().numpy()[good], clean.components.cpu().numpy()[good])
    plan.close()


def test_argument_errors_enqueue_nothing(ctx):
    import torch
    import mav_trajectory_generation_amd as m
    z = C.load("n10_k1_d3")
    plan = m.Plan(ctx, 10, 3, 1, 4, [int(v) for v in z["masks"]])
    t, f = to_device(z["times"], "aos", "times"), to_device(z["d_fixed"], "aos", "fixed")
    for p in (m.TimeObjectiveParams(constraints=[(5, 1.0)]), m.TimeObjectiveParams(time_cost_kind=m.TimeCostKind.kMellingerOuterLoop)):
        with pytest.raises(m.MtgError) as e:
            m.time_objective(plan, t, f, p)
        assert e.value.code == -1
        with pytest.raises(m.MtgError):
            m.magnitude_soft_cost(ctx, torch.zeros((4, 1, 3, 10), dtype=torch.float64, device="cuda"), t[:4].contiguous(), p)
    ctx.sync()
    plan.close()
