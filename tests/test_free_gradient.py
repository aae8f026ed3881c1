"""Gradient with respect to the free derivatives (mtg_free_gradient_host): the library's host form against hand-computed
cases, the independent 50-digit reference (tests/free_gradient_ref.py), the forward map the library already ships (adjoint
identity), the optimum of solveLinear() (stationarity) and the map cost's central differences.  No device.

Bounds (e = 2^-53): every output within e (2 N + 8) sum|terms| of the reference, e (3 N + 12) sum|terms| with coeffs given.
A strict first-order count of the roundings of the rule in include/mtg_hip.h (a power tp_m or tn_m carries m - 1 or m roundings)
gives at most 2 N + 2 without coeffs, inside the constant; with coeffs the same count gives 5 N + 3, above 3 N + 12 for N >= 6:
the test gates on the smaller constant (DESIGN.md section 4.18 has the count).  Largest measured share of the bound over this file: 0.32 without coeffs (N = 10, d = 0), 0.14
with coeffs.  Stationarity at the host solve's optimum: |gradient| / sum|terms| between 1.5e-17 and 5.1e-17; recorded, not
gated.  Chain with the map cost: 1.3e-12 of sum|terms| over ten picks."""
import ctypes
import functools

import mpmath as mp
import numpy as np
import pytest

import mav_trajectory_generation_amd as m
from mav_trajectory_generation_amd import _lib as L
import free_gradient_ref as R
import helpers

E = 2.0 ** -53
ALL_N = (2, 4, 6, 8, 10, 12)
PATTERNS = ("standard", "ends_lower", "interior_free", "interior_full", "none_free", "nothing_fixed")


def pattern_masks(name, N, K):
    """fixed_mask [K + 1] of a pattern, or None where the pattern needs an interior vertex that K = 1 does not have."""
    h = N // 2
    full = (1 << h) - 1
    standard = [full] + [1] * (K - 1) + [full]
    if name == "standard":
        return standard
    if name == "ends_lower":      # ends fixed up to a lower derivative than h - 1 (the reference's test_feasibility.cpp:65-66)
        e = (1 << max(1, h - 1)) - 1
        return [e] + [1] * (K - 1) + [e]
    if name in ("interior_free", "interior_full"):
        if K < 2:
            return None
        out = list(standard)
        out[(K + 1) // 2] = 0 if name == "interior_free" else full
        return out
    if name == "none_free":       # n_free == 0
        return [full] * (K + 1)
    if name == "nothing_fixed":   # n_fixed == 0: structurally rank-deficient for d >= 1
        return [0] * (K + 1)
    raise ValueError(name)


def draw(N, K, D, B, seed):
    rng = np.random.default_rng(seed)
    times = rng.uniform(0.3, 4.0, (B, K))
    return times, rng.standard_normal((B, K, D, N)), rng.standard_normal((B, K, D, N))


def shapes_of(N, d):
    """(pattern, K, D) for one (N, d): every pattern, every K of {1, 2, 3, 8} and every D of {1, 3, 4}, rotated with N and d."""
    out = []
    for i, name in enumerate(PATTERNS):
        ks = [k for k in (1, 2, 3, 8) if pattern_masks(name, N, k) is not None]
        out.append((name, ks[(i + d + N // 2) % len(ks)], (1, 3, 4)[(i + d) % 3]))
    return out


def check_against_reference(N, d, masks, times, grad, coeffs, w, what):
    const = (3 * N + 12) if coeffs is not None else (2 * N + 8)
    gf, gx = m.free_gradient_host(N, d, masks, times, grad, coeffs, w, want_fixed=True)
    ref = R.reference(N, d, masks, times, grad, coeffs, w)
    share = max(R.worst_share(gf, ref["free"], ref["abs_free"], const), R.worst_share(gx, ref["fixed"], ref["abs_fixed"], const))
    print(f"{what}: largest share of e ({const}) sum|terms|: {share:.3e}")
    assert share <= 1.0, (what, share)
    return share


# ---- exact cases ----------------------------------------------------------------------------------------------------------------

def test_n2_by_hand_bit_for_bit():
    """N = 2, K = 1, T = 2: c_0 = x_S, c_1 = (x_E - x_S) / T, so g_S = G_0 - G_1 / 2 and g_E = G_1 / 2; dyadic inputs."""
    G = np.array([[[[0.75, -2.5]], [[3.0, 0.625]]]]).reshape(1, 1, 2, 2)
    for masks in ([1, 0], [0, 1], [0, 0], [1, 1]):
        gf, gx = m.free_gradient_host(2, 0, masks, np.array([[2.0]]), G, want_fixed=True)
        want = {0: G[0, 0, :, 0] - G[0, 0, :, 1] / 2, 1: G[0, 0, :, 1] / 2}
        free = [v for v in (0, 1) if not masks[v]]
        fixed = [v for v in (0, 1) if masks[v]]
        assert gf.shape == (1, 2, len(free)) and gx.shape == (1, 2, len(fixed))
        for c, v in enumerate(free):
            assert np.array_equal(gf[0, :, c], want[v])
        for c, v in enumerate(fixed):
            assert np.array_equal(gx[0, :, c], want[v])


def test_n4_unit_times_integer_input_equals_the_reference_rounded_once():
    """N = 4, K = 2, T = (1, 1): A(1)^-1 has integer entries, every power is 1: with an integer G every operation is exact."""
    rng = np.random.default_rng(4)
    G = rng.integers(-9, 10, (2, 2, 3, 4)).astype(np.float64)
    times = np.ones((2, 2))
    for masks in ([3, 1, 3], [1, 0, 2], [0, 3, 0]):
        gf, gx = m.free_gradient_host(4, 1, masks, times, G, want_fixed=True)
        ref = R.reference(4, 1, masks, times, G)
        assert np.array_equal(gf, R.to_float(ref["free"])) and np.array_equal(gx, R.to_float(ref["fixed"]))


# ---- against the reference ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,d", [(N, d) for N in ALL_N for d in range(N // 2)])
def test_host_form_against_the_reference(N, d):
    for i, (name, K, D) in enumerate(shapes_of(N, d)):
        masks = pattern_masks(name, N, K)
        times, G, c = draw(N, K, D, 2, 1000 * N + 10 * d + i)
        for mode, (g_in, c_in, w) in {"grad": (G, None, 1.0), "coeffs": (None, c, 0.75), "both": (G, c, -1.5)}.items():
            check_against_reference(N, d, masks, times, g_in, c_in, w, f"N={N} d={d} {name} K={K} D={D} {mode}")
        if name == "nothing_fixed" and d >= 1:
            arr = (ctypes.c_uint32 * (K + 1))(*masks)
            assert L.load().mtg_structural_rank_deficiency(N, K, d, arr) > 0


def test_fixed_and_free_together_are_the_pull_back_onto_every_vertex():
    N, d, K, D = 8, 2, 3, 3
    h = N // 2
    times, G, c = draw(N, K, D, 2, 77)
    everything = {}
    for masks in ([0] * (K + 1), [(1 << h) - 1] * (K + 1), [5, 2, 9, 6]):
        gf, gx = m.free_gradient_host(N, d, masks, times, G, c, 0.5, want_fixed=True)
        col, _, _ = R.columns(N, masks)
        full = np.empty((2, D, K + 1, h))
        for (v, p), (kind, cc) in col.items():
            full[:, :, v, p] = (gx if kind == "fixed" else gf)[:, :, cc]
        everything[tuple(masks)] = full
    first = next(iter(everything.values()))
    assert all(np.array_equal(first, x) for x in everything.values())     # the routing moves bits, it computes nothing
    ref = R.reference(N, d, [0] * (K + 1), times, G, c, 0.5)
    assert R.worst_share(first, ref["vertices"], ref["abs_vertices"], 3 * N + 12) <= 1.0


# ---- adjoint identity against the forward map the library ships (its host lane code) ---------------------------------------------

@pytest.mark.parametrize("N", [2, 4, 6, 8, 10])
def test_adjoint_identity_against_the_forward_map(host_emu, N):
    """<J u, w> = <u, J^T w>: J u from the update-from-free path of the solve kernels' lane code with d_fixed = 0."""
    h, K, D, B = N // 2, 3, 3, 4
    d = h - 1
    masks = pattern_masks("standard", N, K) if N > 2 else [1, 0, 0, 1]
    rng = np.random.default_rng(50 + N)
    times = rng.uniform(0.3, 4.0, (B, K))
    n_fixed = helpers.n_fixed(masks)
    n_free = (K + 1) * h - n_fixed
    u = rng.standard_normal((B, D, n_free))
    w = rng.standard_normal((B, K, D, N))
    rc, Ju, _, _, _ = helpers.emu_run(host_emu, N, D, K, d, masks, times, np.zeros((B, D, n_fixed)), mode=2, want_cost=False, d_free_in=u)
    assert rc == 0
    JTw, _ = m.free_gradient_host(N, d, masks, times, w)
    ref = R.reference(N, d, masks, times, w)
    for b in range(B):
        lhs, rhs = float(np.vdot(Ju[b], w[b])), float(np.vdot(u[b], JTw[b]))
        bound = (2 * N + 8) * E * float(sum(abs(x) * s for x, s in zip(u[b].ravel(), ref["abs_free"][b].ravel())))
        tol = 1e-9 * np.linalg.norm(Ju[b]) * np.linalg.norm(w[b]) + bound
        assert abs(lhs - rhs) <= tol, (N, b, lhs, rhs, tol)


# ---- stationarity at the optimum of solveLinear() ---------------------------------------------------------------------------------

@pytest.mark.parametrize("N,d", [(4, 1), (6, 2), (8, 3), (10, 4), (10, 3), (12, 5), (12, 1)])
def test_stationarity_at_the_optimum(host_emu, N, d):
    """The derivative cost's gradient with respect to d_free vanishes at the optimum.  Gate: within the bound of the reference
    evaluated at the same (solved, hence slightly off-optimum) coefficients.  Recorded: |gradient| / sum|terms|."""
    K, D, B = 4, 3, 3
    masks, times, d_fixed = helpers.reference_batch(B, K, N, D, 4242 + N)
    rc, coeffs, _, _, st = helpers.emu_run(host_emu, N, D, K, d, masks, times, d_fixed, mode=0)
    assert rc == 0 and st == 0
    gf, _ = m.free_gradient_host(N, d, masks, times, None, coeffs, 1.0)
    ref = R.reference(N, d, masks, times, None, coeffs, 1.0)
    assert R.worst_share(gf, ref["free"], ref["abs_free"], 3 * N + 12) <= 1.0
    ratio = float(np.max(np.abs(gf) / R.to_float(ref["abs_free"])))
    print(f"N={N} d={d}: |gradient| / sum|terms| at the optimum {ratio:.2e}")
    assert ratio <= 1e-6     # (a sanity line far above the solve's accuracy, not the gate: a wrong transpose gives O(1))


# ---- chain with the map cost ----------------------------------------------------------------------------------------------------

def test_chain_with_the_collision_cost_by_central_differences():
    """Central differences with respect to d_free of the longdouble collision cost of tests/collision_cost_ref.py, the
    coefficients moved through the 50-digit forward map, against free_gradient_host applied to collision_cost_host's gradient.
    Bound 1e-6 sum|terms| (the pull-back of the cost reference's own sum|terms|).  A pick is drawn again when the rounding of the
    two longdouble costs, (S + 16) 2^-64 sum|cost terms| each, divided by the step, exceeds 1 % of the tolerance (the redraw rule
    of the collision cost's own check; it reads the reference's sums only)."""
    import collision_cost_ref as C
    from test_distance_field import DT, H, INFLATION, field_case
    LD = np.longdouble
    eps, seps = 0.5, 1e-3
    coeffs, times, grid, origin = field_case("n10_k8_d3_fast")
    N, K, D, d = 10, coeffs.shape[1], 3, 4
    h = N // 2
    masks = pattern_masks("standard", N, K)
    col, n_fixed, n_free = R.columns(N, masks)
    b = 1
    # vertex derivatives of trajectory b (start of every segment, end of the last) -> a continuous trajectory through the map
    fact = [float(np.prod(np.arange(1, p + 1))) for p in range(h)]
    d_all = np.zeros((D, K + 1, h))
    for v in range(K):
        d_all[:, v, :] = coeffs[b, v, :, :h] * fact
    for p in range(h):
        d_all[:, K, p] = [sum(R.falling(i, p) * coeffs[b, K - 1, a, i] * times[b, K - 1] ** (i - p) for i in range(p, N)) for a in range(D)]
    d_free, d_fixed = np.zeros((D, n_free)), np.zeros((D, n_fixed))
    for (v, p), (kind, c) in col.items():
        (d_fixed if kind == "fixed" else d_free)[:, c] = d_all[:, v, p]
    c0 = R.forward_jacobian_apply(N, masks, times[b], d_free, d_fixed)     # [K][D][N] mpf
    c0_f = R.to_float(c0)[None]
    t_b = times[b:b + 1]
    field = m.DistanceField(grid, origin, H, 0.0)
    r = m.collision_cost_host(c0_f, t_b, field, DT, inflation=INFLATION, epsilon=eps, speed_epsilon=seps)
    got, _ = m.free_gradient_host(N, d, masks, t_b, r.coeff_gradient)
    cref = C.reference(c0_f, t_b, grid, origin, H, 0.0, DT, INFLATION, eps, seps, want_terms=True)
    abs_grad = np.zeros((1, K, D, N))
    abs_grad[:, :, :3, :] = cref["abs_grad"].astype(np.float64)
    scale = R.to_float(R.reference(N, d, masks, t_b, abs_grad)["abs_free"])[0]
    assert not cref["fragile"].any() or cref["fragile"].any(axis=2).sum() <= 1
    inv_col = {c: vp for vp, (kind, c) in col.items() if kind == "free"}
    rng = np.random.default_rng(99)
    worst, done, drawn = 0.0, 0, 0
    while done < 10 and drawn < 200:
        drawn += 1
        a, j = int(rng.integers(D)), int(rng.integers(n_free))
        v, p = inv_col[j]
        segs = [k for k in (v - 1, v) if 0 <= k < K]
        if scale[a, j] == 0.0 or cref["fragile"][0, segs].any():
            continue
        step = 1e-6 / max(1.0, float(times[b, segs].max()) ** p)
        noise = sum((float(cref["S"][0, k]) + 16.0) * 2.0 ** -64 * float(cref["abs_cost"][0, k]) for k in segs) / step
        if noise > 1e-8 * scale[a, j]:
            continue
        unit = np.zeros((D, n_free))
        unit[a, j] = 1.0
        col_j = R.forward_jacobian_apply(N, masks, times[b], unit, np.zeros((D, n_fixed)))     # J e_j, exact to 50 digits
        cost = []
        for sign in (1, -1):
            c = np.array([[LD(float(c0[k, q, i])) + LD(float(c0[k, q, i] - mp.mpf(float(c0[k, q, i]))))
                           + sign * LD(step) * LD(float(col_j[k, q, i])) for i in range(N)] for k in segs for q in range(D)],
                         dtype=LD).reshape(1, len(segs), D, N)
            cost.append(C.reference(c, t_b[:, segs], grid, origin, H, 0.0, DT, INFLATION, eps, seps)["cost"][0].sum())
        fd = float((cost[0] - cost[1]) / (2 * LD(step)))
        worst = max(worst, abs(fd - got[0, a, j]) / scale[a, j])
        done += 1
    print(f"chain: {done} picks of {drawn} drawn, largest |central difference - pulled-back gradient| / sum|terms| {worst:.2e}")
    assert done == 10
    assert worst <= 1e-6


# ---- buffers and layouts --------------------------------------------------------------------------------------------------------

def raw_call(N, d, masks, times, grad, coeffs, w, D, want_free=True, want_fixed=True, gap=1, ts=None):
    """The C entry itself on NaN-filled buffers with `gap` elements between columns and guard words at both ends: returns the
    whole buffers."""
    lib = L.load()
    K, h = len(masks) - 1, N // 2
    B = times.shape[0]
    n_fixed = helpers.n_fixed([mk & ((1 << h) - 1) for mk in masks])
    n_free = h * (K + 1) - n_fixed
    guard = 3
    lay = L.Layout()
    lay.times_stride_b, lay.times_stride_k = ts or (K, 1)
    lay.fixed_stride_b, lay.fixed_stride_d, lay.fixed_stride_c = D * n_fixed * gap, n_fixed * gap, gap
    lay.free_stride_b, lay.free_stride_d, lay.free_stride_c = D * n_free * gap, n_free * gap, gap
    free = np.full(guard + B * D * n_free * gap + guard, np.nan)
    fixed = np.full(guard + B * D * n_fixed * gap + guard, np.nan)
    desc = L.PlanDesc(N, D, K, d, (ctypes.c_uint32 * (K + 1))(*masks))
    p = lambda a, off=0: ctypes.c_void_p(0) if a is None else ctypes.c_void_p(a.ctypes.data + 8 * off)
    rc = lib.mtg_free_gradient_host(ctypes.byref(desc), B, ctypes.byref(lay), p(np.ascontiguousarray(times)), p(grad), p(coeffs), w,
                                    p(free if want_free else None, guard), p(fixed if want_fixed else None, guard))
    assert rc == 0
    return free, fixed, guard, n_free, n_fixed


@pytest.mark.parametrize("want", [(True, True), (True, False), (False, True)])
def test_optional_outputs_guard_words_and_gaps(want):
    N, d, K, D, B = 6, 1, 3, 4, 3
    masks = [7, 1, 0, 3]
    times, G, c = draw(N, K, D, B, 5)
    dense_f, dense_x = m.free_gradient_host(N, d, masks, times, G, c, 2.0, want_fixed=True)
    for gap in (1, 2):
        free, fixed, guard, n_free, n_fixed = raw_call(N, d, masks, times, G, c, 2.0, D, want[0], want[1], gap)
        for buf, wanted, dense, n in ((free, want[0], dense_f, n_free), (fixed, want[1], dense_x, n_fixed)):
            body = buf[guard:len(buf) - guard].reshape(B, D, n, gap)
            assert np.isnan(buf[:guard]).all() and np.isnan(buf[len(buf) - guard:]).all()
            assert np.isnan(body[..., 1:]).all()                  # the gaps between the columns stay untouched
            if wanted:
                assert np.array_equal(body[..., 0], dense)
            else:
                assert np.isnan(body).all()


def test_no_free_columns_and_a_null_grad_free():
    N, d, K, D = 4, 0, 2, 3
    times, G, _ = draw(N, K, D, 2, 6)
    free, fixed, guard, n_free, n_fixed = raw_call(N, d, [3, 3, 3], times, G, None, 0.0, D, want_free=False)
    assert n_free == 0 and not np.isnan(fixed[guard:len(fixed) - guard]).any()
    gf, gx = m.free_gradient_host(N, d, [3, 3, 3], times, G, want_fixed=True)
    assert gf.shape == (2, D, 0) and np.array_equal(gx.ravel(), fixed[guard:len(fixed) - guard])


@pytest.mark.parametrize("mode", ["grad", "coeffs", "both"])
def test_soa_outputs_and_k_b_times_equal_aos(mode):
    N, d, K, D, B = 10, 4, 8, 3, 5
    masks = pattern_masks("standard", N, K)
    times, G, c = draw(N, K, D, B, 8)
    g_in, c_in = (G if mode != "coeffs" else None), (c if mode != "grad" else None)
    af, ax = m.free_gradient_host(N, d, masks, times, g_in, c_in, 0.3, want_fixed=True)
    sf, sx = m.free_gradient_host(N, d, masks, np.ascontiguousarray(times.T), g_in, c_in, 0.3, layout="soa", want_fixed=True)
    assert sf.shape == (D, af.shape[2], B) and sx.shape == (D, ax.shape[2], B)
    assert np.array_equal(sf.transpose(2, 0, 1), af) and np.array_equal(sx.transpose(2, 0, 1), ax)


def test_zero_weight_with_coeffs_equals_the_call_without_coeffs():
    N, d, K, D = 8, 2, 3, 4
    masks = pattern_masks("ends_lower", N, K)
    times, G, c = draw(N, K, D, 3, 9)
    a = m.free_gradient_host(N, d, masks, times, G, c, 0.0, want_fixed=True)
    b = m.free_gradient_host(N, d, masks, times, G, None, 123.0, want_fixed=True)     # (the weight is ignored without coeffs)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_special_times_touch_their_own_trajectory_only():
    """Times are not validated: T = 0 and a NaN T give what the arithmetic gives, in their own rows."""
    N, d, K, D, B = 6, 2, 3, 3, 4
    masks = pattern_masks("standard", N, K)
    times, G, c = draw(N, K, D, B, 10)
    clean = m.free_gradient_host(N, d, masks, times, G, c, 1.0, want_fixed=True)
    bad = times.copy()
    bad[1, 1], bad[2, 0] = 0.0, np.nan
    got = m.free_gradient_host(N, d, masks, bad, G, c, 1.0, want_fixed=True)
    for x, y in zip(clean, got):
        assert np.array_equal(x[[0, 3]], y[[0, 3]])
        assert not np.isfinite(y[1]).all() and np.isnan(y[2]).any()
