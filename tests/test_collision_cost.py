"""Distance-field collision cost and gradient (mtg_collision_cost): the independent longdouble reference against itself (central
differences, a case written by hand) and the library's host form against it.  No device."""
import ctypes
import functools

import numpy as np
import pytest

import mav_trajectory_generation_amd as m
from mav_trajectory_generation_amd import _lib as L
import collision_cost_ref as C
import distance_field_ref as R
from test_distance_field import CASES, DT, H, INFLATION, field_case

EPSILON, SPEED_EPSILON = 0.5, 1e-3
LD = np.longdouble


@functools.lru_cache(maxsize=None)
def reference_of(name, outside=0.0):
    coeffs, times, grid, origin = field_case(name)
    return C.reference(coeffs, times, grid, origin, H, outside, DT, INFLATION, EPSILON, SPEED_EPSILON, want_terms=True)


def host(name, outside=0.0, layout="aos", **kw):
    coeffs, times, grid, origin = field_case(name)
    t = times if layout == "aos" else np.ascontiguousarray(times.T)
    return m.collision_cost_host(coeffs, t, m.DistanceField(grid, origin, H, outside), DT, inflation=INFLATION, epsilon=EPSILON,
                                 speed_epsilon=SPEED_EPSILON, times_layout=layout, **kw)


def compare(ref, r, what, special=None):
    """r (a CollisionCostResult of numpy arrays) against a reference: every output of every segment without a fragile sample
    within its a-priori bound; at most 1 % of the segments left out.  special: segments whose values the rule states outright
    (a time that is not positive, the cap), which the caller compares itself.  Returns the largest share of the bound."""
    fragile = ref["fragile"].any(axis=2)
    assert fragile.sum() <= 0.01 * fragile.size, (what, int(fragile.sum()))
    ok = ~fragile if special is None else ~fragile & ~special
    assert np.array_equal(r.segment_samples[ok], ref["S"].astype(np.int32)[ok])
    err = np.abs(r.segment_cost.astype(LD) - ref["cost"]).astype(np.float64)
    share = float((err[ok] / np.maximum(ref["bound_cost"][ok], 1e-300)).max())
    rel = float((err[ok] / np.maximum(ref["abs_cost"][ok].astype(np.float64), 1e-300)).max())
    assert (err[ok] <= ref["bound_cost"][ok]).all(), (what, share)
    gshare = grel = 0.0
    if r.coeff_gradient is not None:
        gerr = np.abs(r.coeff_gradient[:, :, :3, :].astype(LD) - ref["grad"]).astype(np.float64)
        gshare = float((gerr[ok] / np.maximum(ref["bound_grad"][ok], 1e-300)).max())
        grel = float((gerr[ok] / np.maximum(ref["abs_grad"][ok].astype(np.float64), 1e-300)).max())
        assert (gerr[ok] <= ref["bound_grad"][ok]).all(), (what, gshare)
        assert (r.coeff_gradient[:, :, 3:, :] == 0.0).all()
    print(f"{what}: {ref['samples']} samples, {ref['positive']} with c > 0, {int(fragile.sum())} of {fragile.size} segments excluded, "
          f"smallest |u - integer| inside {ref['u_gap']:.2e}; largest share of the bound: cost {share:.3e}, gradient {gshare:.3e}; "
          f"largest error / sum|terms|: cost {rel:.2e}, gradient {grel:.2e}")
    return max(share, gshare)


# ---- the reference itself, without the library ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_reference_gradient_is_the_central_difference_of_the_reference_cost(name):
    """Three dozen seeded (trajectory, segment, axis, power) picks; step 1e-7 / max(1, T^j); within 1e-6 sum |terms| of the entry
    (the cost is piecewise C^2: the residue is the jump of the second derivative at the potential's joints).
    A difference quotient has to be resolvable in the arithmetic that forms it: the two longdouble costs carry about
    (S + 16) 2^-64 sum |cost terms| of rounding each, which the division by 2 step magnifies.  A pick is drawn again if that
    exceeds 1 % of the tolerance (an entry of a high power whose only costly samples lie at small t: t^j and the step are both
    tiny); the criterion reads the reference's sums only, never the difference itself."""
    coeffs, times, grid, origin = field_case(name)
    ref = reference_of(name)
    rng = np.random.default_rng(1717 + CASES.index(name))
    live = np.argwhere((ref["abs_cost"] > 0) & ~ref["fragile"].any(axis=2))
    worst, done, drawn = 0.0, 0, 0
    while done < 36 and drawn < 400:
        drawn += 1
        b, k = live[rng.integers(len(live))]
        a, j = int(rng.integers(3)), int(rng.integers(coeffs.shape[-1]))
        step = LD(1e-7) / LD(max(1.0, times[b, k] ** j))
        scale = ref["abs_grad"][b, k, a, j]
        noise = (float(ref["S"][b, k]) + 16.0) * 2.0 ** -64 * float(ref["abs_cost"][b, k]) / float(step)
        if noise > 1e-8 * float(scale):
            continue
        done += 1
        cost = []
        for sign in (1, -1):
            c = coeffs[b:b + 1, k:k + 1].astype(LD)
            c[0, 0, a, j] += sign * step
            cost.append(C.reference(c, times[b:b + 1, k:k + 1], grid, origin, H, 0.0, DT, INFLATION, EPSILON, SPEED_EPSILON)["cost"][0, 0])
        fd = (cost[0] - cost[1]) / (2 * step)
        worst = max(worst, float(abs(fd - ref["grad"][b, k, a, j]) / scale))
    print(f"{name}: {done} picks of {drawn} drawn, largest |central difference - gradient| / sum |terms| {worst:.2e}")
    assert done == 36
    assert worst <= 1e-6


NX, NY, NZ = 8, 6, 4


def linear_field(axis, outside=4.0):
    """d = x, 2 y or 3 z on an 8 x 6 x 4 grid with origin 0 and h = 0.5 (exact in float32: multiples of 1/2)."""
    iz, iy, ix = np.meshgrid(np.arange(NZ), np.arange(NY), np.arange(NX), indexing="ij")
    return ((ix, iy, iz)[axis] * 0.5 * (axis + 1)).astype(np.float32)


def hand_case(axis):
    """Field d = (axis + 1) p_axis, a straight segment at constant speed along x: p = (0.5 + 0.5 t, 0.5, 0.25), T = 2, dt = 0.5:
    samples t = 0, 0.5, .. 2 (S = 5), weights 0.25, 0.5, 0.5, 0.5, 0.25, s = 0.5 with speed_epsilon = 0.  With epsilon = 1 and
    inflation = 0.25 every number below is a small dyadic rational: exact in float64."""
    coeffs = np.zeros((1, 1, 3, 2))
    coeffs[0, 0, :, 0] = (0.5, 0.5, 0.25)
    coeffs[0, 0, 0, 1] = 0.5
    t = np.array([0.0, 0.5, 1.0, 1.5, 2.0])
    w = np.array([0.25, 0.5, 0.5, 0.5, 0.25])
    pos = np.stack([0.5 + 0.5 * t, np.full(5, 0.5), np.full(5, 0.25)], axis=1)
    x = (axis + 1) * pos[:, axis] - 0.25
    c = np.where(x < 0, 0.5 - x, np.where(x <= 1.0, (x - 1.0) ** 2 / 2.0, 0.0))
    dc = np.where(x < 0, -1.0, np.where(x <= 1.0, x - 1.0, 0.0))
    s = 0.5
    cost = (w * c * s).sum()
    grad = np.zeros((3, 2))
    G = np.zeros(3)
    G[axis] = axis + 1.0
    for a in range(3):
        for j in range(2):
            direction = (0.5 if a == 0 else 0.0) / s * (1.0 if j == 1 else 0.0)
            grad[a, j] = (w * dc * s * G[a] * t ** j + w * c * direction).sum()
    return coeffs, np.array([[2.0]]), cost, grad


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_reference_on_a_linear_field_by_hand(axis):
    coeffs, times, cost, grad = hand_case(axis)
    ref = C.reference(coeffs, times, linear_field(axis), (0.0, 0.0, 0.0), 0.5, 4.0, 0.5, 0.25, 1.0, 0.0)
    assert ref["S"][0, 0] == 5 and cost > 0
    assert float(ref["cost"][0, 0]) == cost
    assert np.array_equal(ref["grad"][0, 0].astype(np.float64), grad)


# ---- the host form --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axis", [0, 1, 2])
def test_host_on_a_linear_field_by_hand(axis):
    coeffs, times, cost, grad = hand_case(axis)
    r = m.collision_cost_host(coeffs, times, m.DistanceField(linear_field(axis), (0.0, 0.0, 0.0), 0.5, 4.0), 0.5, inflation=0.25,
                              epsilon=1.0, speed_epsilon=0.0)
    assert r.segment_samples[0, 0] == 5
    assert r.segment_cost[0, 0] == cost and r.trajectory_cost[0] == cost
    assert np.array_equal(r.coeff_gradient[0, 0], grad)


@pytest.mark.parametrize("outside", [0.0, np.inf])
@pytest.mark.parametrize("name", CASES)
def test_host_form_against_the_reference(name, outside):
    """Measured largest shares of the bound: DESIGN.md section 4.17."""
    ref = reference_of(name, outside)
    assert 0 < ref["positive"] < ref["samples"]
    compare(ref, host(name, outside), f"{name} outside={outside}")


@pytest.mark.parametrize("name", CASES)
def test_sample_counts_trajectory_cost_and_cost_only(name):
    coeffs, times, _, _ = field_case(name)
    r, r0 = host(name), host(name, want_gradient=False)
    assert np.array_equal(r.segment_samples, R.sample_counts(times, DT).astype(np.int32))
    total = np.zeros(len(coeffs))
    for k in range(times.shape[1]):
        total = total + r.segment_cost[:, k]
    assert np.array_equal(r.trajectory_cost, total)
    assert r0.coeff_gradient is None
    assert np.array_equal(r0.segment_cost, r.segment_cost) and np.array_equal(r0.trajectory_cost, r.trajectory_cost)
    assert np.array_equal(r0.segment_samples, r.segment_samples)


def test_times_as_k_b_equal_b_k():
    a, b = host("n12_k4_d4"), host("n12_k4_d4", layout="soa")
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_yaw_rows_are_zero_and_yaw_is_never_read():
    coeffs, times, grid, origin = field_case("n7_k4_d4")
    assert coeffs.shape[2] == 4
    f = m.DistanceField(grid, origin, H, 0.0)
    kw = dict(inflation=INFLATION, epsilon=EPSILON, speed_epsilon=SPEED_EPSILON)
    a = m.collision_cost_host(coeffs, times, f, DT, **kw)
    other = coeffs.copy()
    other[:, :, 3, :] = np.random.default_rng(5).normal(size=other[:, :, 3, :].shape) * 1e6
    other[0, 0, 3, 0] = np.nan
    b = m.collision_cost_host(other, times, f, DT, **kw)
    assert (a.coeff_gradient[:, :, 3, :] == 0.0).all() and np.abs(a.coeff_gradient[:, :, :3, :]).max() > 0
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    c = m.collision_cost_host(np.ascontiguousarray(coeffs[:, :, :3, :]), times, f, DT, **kw)
    assert np.array_equal(c.coeff_gradient, a.coeff_gradient[:, :, :3, :]) and np.array_equal(c.segment_cost, a.segment_cost)


def test_segment_times_that_are_not_positive_and_the_cap():
    """T = 0 and T < 0: cost 0, gradient 0, S = 2.  T NaN: NaN, S = 2.  S > max_samples: NaN, -1.  The yaw rows: 0 throughout."""
    coeffs, times, grid, origin = field_case("n7_k4_d4")
    coeffs, times = coeffs[:2].copy(), times[:2].copy()
    times[0, 0], times[0, 1], times[0, 2], times[1, 3] = 0.0, -0.5, np.nan, 299.5 * DT
    f = m.DistanceField(grid, origin, H, 0.0)
    r = m.collision_cost_host(coeffs, times, f, DT, inflation=INFLATION, epsilon=EPSILON, speed_epsilon=SPEED_EPSILON, max_samples=300)
    assert R.sample_counts(times, DT)[1, 3] == 301 and R.sample_counts(field_case("n7_k4_d4")[1], DT).max() < 300
    assert list(r.segment_samples[0, :3]) == [2, 2, 2] and r.segment_samples[1, 3] == -1
    for k in (0, 1):
        assert r.segment_cost[0, k] == 0.0 and (r.coeff_gradient[0, k] == 0.0).all()
    assert np.isnan(r.segment_cost[0, 2]) and np.isnan(r.coeff_gradient[0, 2, :3]).all()
    assert np.isnan(r.segment_cost[1, 3]) and np.isnan(r.coeff_gradient[1, 3, :3]).all()
    assert (r.coeff_gradient[:, :, 3] == 0.0).all()
    assert np.isnan(r.trajectory_cost).all()
    # the other segments are what they are without those four
    clean = m.collision_cost_host(coeffs, field_case("n7_k4_d4")[1][:2], f, DT, inflation=INFLATION, epsilon=EPSILON,
                                  speed_epsilon=SPEED_EPSILON)
    keep = np.ones((2, 4), dtype=bool)
    keep[0, :3] = keep[1, 3] = False
    assert np.array_equal(r.segment_cost[keep], clean.segment_cost[keep])
    assert np.array_equal(r.coeff_gradient[keep], clean.coeff_gradient[keep])
    # S == max_samples is sampled
    r = m.collision_cost_host(coeffs, times, f, DT, inflation=INFLATION, epsilon=EPSILON, speed_epsilon=SPEED_EPSILON, max_samples=301)
    assert r.segment_samples[1, 3] == 301 and np.isfinite(r.segment_cost[1, 3])


def test_a_trajectory_wholly_outside_the_grid():
    """Every sample takes outside_distance: the cost is sum w c(outside - inflation) s and the gradient has the direction term
    only (G = 0)."""
    rng = np.random.default_rng(77)
    coeffs = rng.normal(size=(2, 2, 3, 6))
    coeffs[:, :, :, 0] += 1000.0
    times = np.array([[1.3, 0.7], [2.1, 0.4]])
    grid = linear_field(0)
    outside, inflation, eps, eta, dt = 0.375, 0.125, 0.5, 1e-3, 0.05
    r = m.collision_cost_host(coeffs, times, m.DistanceField(grid, (0.0, 0.0, 0.0), 0.5, outside), dt, inflation=inflation, epsilon=eps,
                              speed_epsilon=eta)
    ref = C.reference(coeffs, times, grid, (0.0, 0.0, 0.0), 0.5, outside, dt, inflation, eps, eta, want_terms=True)
    assert not ref["fragile"].any()
    compare(ref, r, "outside")
    # by hand: c is one number
    c = (outside - inflation - eps) ** 2 / (2 * eps)
    t, w, valid = ref["t"], ref["w"], ref["valid"]
    N = coeffs.shape[-1]
    j = np.arange(N)
    v = sum(j[i] * coeffs[:, :, None, :, i] * t[..., None] ** max(i - 1, 0) for i in range(1, N))       # [B][K][S][3]
    s = np.sqrt((v * v).sum(axis=-1) + eta * eta)
    want = np.where(valid, w * c * s, 0.0).sum(axis=2)
    assert np.allclose(r.segment_cost, want, rtol=1e-12, atol=0)
    dpw = np.where(j >= 1, j * t[..., None] ** np.maximum(j - 1, 0), 0.0)                                # [B][K][S][N]
    gwant = np.where(valid[..., None, None], (w * c / s)[..., None, None] * v[..., None] * dpw[..., None, :], 0.0).sum(axis=2)
    assert np.allclose(r.coeff_gradient, gwant, rtol=1e-10, atol=1e-14)
    assert (r.coeff_gradient[:, :, :, 0] == 0.0).all()
    # outside = +infinity: free space costs nothing
    r = m.collision_cost_host(coeffs, times, m.DistanceField(grid, (0.0, 0.0, 0.0), 0.5, np.inf), dt, inflation=inflation, epsilon=eps)
    assert (r.segment_cost == 0.0).all() and (r.coeff_gradient == 0.0).all()


def test_doubling_speed_epsilon_on_a_resting_end():
    """s(2 eta) - s(eta) <= eta at every sample, so the cost grows by no more than sum w c eta (and does grow)."""
    coeffs, times, grid, origin = field_case("n10_k8_d3_fast")
    f = m.DistanceField(grid, origin, H, 0.0)
    eta = 0.05
    kw = dict(inflation=INFLATION, epsilon=EPSILON)
    a = m.collision_cost_host(coeffs, times, f, DT, speed_epsilon=eta, **kw)
    b = m.collision_cost_host(coeffs, times, f, DT, speed_epsilon=2 * eta, **kw)
    ref = C.reference(coeffs, times, grid, origin, H, 0.0, DT, INFLATION, EPSILON, eta, want_terms=True)
    # sum w c: the reference's terms over its speeds
    vel = np.zeros(ref["t"].shape + (3,))
    for i in range(coeffs.shape[-1] - 1, 0, -1):
        vel = vel * ref["t"][..., None] + i * coeffs[:, :, None, :3, i]
    s = np.sqrt((vel * vel).sum(axis=-1) + eta * eta)
    wc = np.where(ref["valid"], ref["terms"] / s, 0.0).sum(axis=2)
    first = a.segment_cost[:, 0] > 0      # the first segment starts at rest
    assert first.any()
    growth = b.segment_cost - a.segment_cost
    assert (growth >= 0).all() and (growth[:, 0][first] > 0).all()
    assert (growth <= wc * eta * (1 + 1e-9) + 1e-15).all()


def straight_segments(lengths, dt, n=6):
    """One trajectory per sample count S in `lengths`, K = 1, n coefficients: a curved path through the linear field's grid, T
    chosen so that the segment has exactly S samples."""
    rng = np.random.default_rng(99)
    B = len(lengths)
    times = np.array([[(S - 2 + 0.5) * dt] for S in lengths])
    coeffs = np.zeros((B, 1, 3, max(n, 6)))
    for b in range(B):
        T = times[b, 0]
        start, end = rng.uniform([0.3, 0.3, 0.2], [1.0, 1.0, 0.5]), rng.uniform([2.2, 1.6, 0.9], [3.2, 2.2, 1.3])
        coeffs[b, 0, :, 0] = start
        coeffs[b, 0, :, 1] = (end - start) / T
        coeffs[b, 0, :, 2] = rng.normal(size=3) * 0.3 / T ** 2
        coeffs[b, 0, :, 3] = -coeffs[b, 0, :, 2] / T
        for i in range(6, n):
            coeffs[b, 0, :, i] = rng.normal(size=3) * 0.02 / T ** i
    return coeffs, times


@pytest.mark.parametrize("dt", [0.05, 0.013])
def test_sample_counts_around_the_partition(dt):
    lengths = (2, 3, 63, 64, 65, 129, 200)
    coeffs, times = straight_segments(lengths, dt)
    assert list(R.sample_counts(times, dt)[:, 0]) == list(lengths)
    grid = (linear_field(0) * 0.25 + linear_field(1) * 0.125 + linear_field(2) * 0.0625).astype(np.float32)
    ref = C.reference(coeffs, times, grid, (0.0, 0.0, 0.0), 0.5, 0.0, dt, 0.125, 0.75, 1e-3)
    assert (ref["abs_cost"] > 0).all()
    r = m.collision_cost_host(coeffs, times, m.DistanceField(grid, (0.0, 0.0, 0.0), 0.5, 0.0), dt, inflation=0.125, epsilon=0.75)
    compare(ref, r, f"S = {lengths}, dt = {dt}")


@pytest.mark.parametrize("name", CASES)
def test_the_order_of_summation_restated(name):
    """The 64 partial sums and the butterfly, in Python, on the reference's terms rounded to float64: the host's sums differ from
    it only by the errors of the terms themselves (bound_terms) and a few ulps of sum |terms|, not by the summation part of the
    bound.  A wrong partition or a dropped lane moves a sum by whole terms."""
    ref = reference_of(name)
    r = host(name)
    ok = ~ref["fragile"].any(axis=2)
    ulps = 8 * C.EPS
    got = C.butterfly(ref["terms"])
    assert (np.abs(got - r.segment_cost)[ok] <= (ref["bound_terms_cost"] + ulps * ref["abs_cost"].astype(np.float64))[ok]).all()
    ggot = C.butterfly(np.moveaxis(ref["grad_terms"], 2, -1))
    lim = ref["bound_terms_grad"] + ulps * ref["abs_grad"].astype(np.float64)
    assert (np.abs(ggot - r.coeff_gradient[:, :, :3, :])[ok] <= lim[ok]).all()
    # and the restatement is itself a sum of these terms
    assert np.allclose(got, ref["terms"].sum(axis=2), rtol=1e-12, atol=0)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 9, 11])
def test_odd_and_small_n_equal_the_padded_even_form(n):
    coeffs, times = straight_segments((3, 64, 65), 0.05, n)
    coeffs = np.ascontiguousarray(coeffs[:, :, :, :n])
    grid = (linear_field(0) * 0.25 + linear_field(1) * 0.125).astype(np.float32)
    f = m.DistanceField(grid, (0.0, 0.0, 0.0), 0.5, 0.0)
    a = m.collision_cost_host(coeffs, times, f, 0.05, inflation=0.125, epsilon=0.75)
    padded = np.zeros(coeffs.shape[:3] + (n + 1,))
    padded[..., :n] = coeffs
    b = m.collision_cost_host(padded, times, f, 0.05, inflation=0.125, epsilon=0.75)
    assert np.array_equal(a.segment_cost, b.segment_cost) and (a.segment_cost > 0).all()
    assert np.array_equal(a.coeff_gradient, b.coeff_gradient[..., :n])


def field_struct(grid, origin, h, outside=0.0, interpolation=1):
    nz, ny, nx = grid.shape
    return L.DistanceFieldC(grid.ctypes.data, nx, ny, nz, (ctypes.c_double * 3)(*origin), h, outside, interpolation)


def test_optional_outputs_in_every_combination_and_guard_words():
    coeffs, times, grid, origin = field_case("n7_k4_d4")
    coeffs, times = np.ascontiguousarray(coeffs[:5]), np.ascontiguousarray(times[:5])
    B, K, D, N = coeffs.shape
    lib = L.load()
    fc = field_struct(grid, origin, H)
    full = m.collision_cost_host(coeffs, times, m.DistanceField(grid, origin, H, 0.0), DT, inflation=INFLATION, epsilon=EPSILON)
    want = dict(seg=full.segment_cost, traj=full.trajectory_cost, grad=full.coeff_gradient, samples=full.segment_samples)
    guard = 3
    for mask in range(8):
        bufs = {}
        for bit, (key, shape, dtype) in enumerate((("traj", (B,), np.float64), ("grad", (B, K, D, N), np.float64), ("samples", (B, K), np.int32))):
            if mask >> bit & 1:
                bufs[key] = np.full(int(np.prod(shape)) + 2 * guard, -77, dtype=dtype)
        bufs["seg"] = np.full(B * K + 2 * guard, -77.0)
        ptr = lambda key: bufs[key][guard:].ctypes.data if key in bufs else None
        rc = lib.mtg_collision_cost_host(N, K, D, B, coeffs.ctypes.data, times.ctypes.data, K, 1, ctypes.byref(fc), DT, 4096, INFLATION,
                                         EPSILON, SPEED_EPSILON, ptr("seg"), ptr("traj"), ptr("grad"), ptr("samples"))
        assert rc == 0
        for key, buf in bufs.items():
            assert (buf[:guard] == -77).all() and (buf[-guard:] == -77).all(), (mask, key)
            assert np.array_equal(buf[guard:-guard], want[key].ravel()), (mask, key)


def test_a_single_trajectory_comes_without_the_batch_axis():
    coeffs, times, grid, origin = field_case("n5_k3_d3")
    f = m.DistanceField(grid, origin, H, 0.0)
    kw = dict(inflation=INFLATION, epsilon=EPSILON)
    one, many = m.collision_cost_host(coeffs[3], times[3], f, DT, **kw), m.collision_cost_host(coeffs, times, f, DT, **kw)
    assert one.trajectory_cost.shape == () and one.coeff_gradient.shape == coeffs.shape[1:]
    assert all(np.array_equal(x, y[3]) for x, y in zip(one, many))


def test_names_resolve_lazily_and_are_exported():
    assert m.collision_cost_host is m.segment_checks.collision_cost_host and m.CollisionCostResult._fields == (
        "trajectory_cost", "segment_cost", "coeff_gradient", "segment_samples")
    assert "collision_cost" not in dir(m)
    lib = L.load()
    assert lib.mtg_collision_cost and lib.mtg_collision_cost_host


def test_no_instantiation_uses_scratch(tmp_path):
    """The kernel's translation unit compiled for the device with the build's own flags and the resource remarks on: ten segment
    kernels (NC = 4 .. 12, with and without the gradient) and the per-trajectory sum; none uses scratch or LDS, and the cost-only
    instantiation needs fewer registers than its twin."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import __graft_entry__ as g
    src = os.path.join(g.CSRC, "mtg_collision.hip")
    r = subprocess.run(["hipcc"] + g.HIP_FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                                                  str(tmp_path / "mtg_collision.o")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    found = {}
    for name, body in re.findall(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", r.stderr, flags=re.S):
        get = lambda key: int(re.search(re.escape(key) + r": (\d+)", body).group(1))
        found[name] = (get("VGPRs"), get("AGPRs"), get("ScratchSize [bytes/lane]"), get("LDS Size [bytes/block]"))
    seg = {k: v for k, v in found.items() if "collision_seg_kernel" in k}
    assert len(seg) == 10 and any("collision_traj_kernel" in k for k in found), sorted(found)
    assert all(v[2] == 0 and v[3] == 0 for v in found.values()), found
    for nc in (4, 6, 8, 10, 12):
        with_gradient = [v for k, v in seg.items() if f"ILi{nc}ELb1E" in k][0]
        cost_only = [v for k, v in seg.items() if f"ILi{nc}ELb0E" in k][0]
        assert cost_only[0] + cost_only[1] < with_gradient[0] + with_gradient[1]
    print({k[-30:]: v for k, v in seg.items()})
