"""Gradient with respect to the free derivatives on the device (mtg_free_gradient): every instantiation, D in {1, 3, 4}, chain
lengths 1, 2, 3, 8, batches 1, 3 and 65 (65 x (K + 1) D lanes cross wavefront and workgroup boundaries at an odd offset), the mask
patterns of tests/test_free_gradient.py, both output layouts, [K][B] times, NaN-filled guarded buffers and the three input
combinations: every call against the host form bit for bit; one case per N against the 50-digit reference; the adjoint identity
against Plan.update_from_free; T = 0 and a NaN time in a batch of ordinary ones; the argument table with a real plan."""
import ctypes

import numpy as np
import pytest

import free_gradient_ref as R
from test_free_gradient import ALL_N, E, PATTERNS, draw, pattern_masks

pytestmark = pytest.mark.gpu
GUARD = 4


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import mav_trajectory_generation_amd as m
    c = m.Context(0)
    yield c
    c.close()


def same_bits(a, b):
    """Bit for bit; where the host has a NaN the device has a NaN (its sign and payload are the processor's, not the rule's)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def device_call(ctx, plan, times, grad, coeffs, w, layout="aos", want_free=True, want_fixed=True):
    """mtg_free_gradient into NaN-filled buffers between guard words; (grad_free, grad_fixed) in `layout` as numpy arrays, None
    for an output that was not asked for (its buffer must then be untouched)."""
    import torch
    from mav_trajectory_generation_amd import _lib as L
    B = times.shape[0]
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t_d = dev(times if layout == "aos" else times.T)
    g_d, c_d = dev(grad), dev(coeffs)
    bufs = [torch.full((B * plan.D * n + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda") for n in (plan.n_free, plan.n_fixed)]
    ptr = lambda t, off=0: ctypes.c_void_p(0) if t is None else ctypes.c_void_p(t.data_ptr() + 8 * off)
    lay = plan.layout(B, layout)
    cur = ctx._enter()
    rc = ctx.lib.mtg_free_gradient(plan.handle, B, ctypes.byref(lay), ptr(t_d), ptr(g_d), ptr(c_d), float(w),
                                   ptr(bufs[0] if want_free else None, GUARD), ptr(bufs[1] if want_fixed else None, GUARD))
    ctx._leave(cur)
    assert rc == 0, ctx.lib.mtg_last_error_string(ctx.handle)
    ctx.sync()
    out = []
    for buf, n, wanted in zip(bufs, (plan.n_free, plan.n_fixed), (want_free, want_fixed)):
        h = buf.cpu().numpy()
        assert np.isnan(h[:GUARD]).all() and np.isnan(h[len(h) - GUARD:]).all()
        body = h[GUARD:len(h) - GUARD]
        if not wanted:
            assert np.isnan(body).all()
            out.append(None)
        else:
            out.append(body.reshape((B, plan.D, n) if layout == "aos" else (plan.D, n, B)))
    return out


def host_call(plan, times, grad, coeffs, w, layout="aos"):
    import mav_trajectory_generation_amd as m
    t = times if layout == "aos" else np.ascontiguousarray(times.T)
    return m.free_gradient_host(plan.N, plan.deriv, plan.fixed_mask, t, grad, coeffs, w, layout=layout, want_fixed=True, dimension=plan.D)


@pytest.mark.parametrize("N", ALL_N)
def test_every_instance_against_the_host_form_and_the_reference(ctx, N):
    import torch
    import mav_trajectory_generation_amd as m
    h = N // 2
    checked_reference = False
    for i, name in enumerate(PATTERNS):
        ks = [k for k in (1, 2, 3, 8) if pattern_masks(name, N, k) is not None]
        K, D, B, d = ks[(i + h) % len(ks)], (1, 3, 4)[(i + h) % 3], (1, 3, 65)[(i + N) % 3], (i + h) % h
        masks = pattern_masks(name, N, K)
        plan = m.Plan(ctx, N, D, K, d, masks)
        times, G, c = draw(N, K, D, B, 31 * N + i)
        for j, (g_in, c_in, w) in enumerate(((G, None, 1.0), (None, c, 0.75), (G, c, -1.5))):
            layout = ("aos", "soa")[(i + j) % 2]
            want = (True, True) if j != 1 else ((True, False) if i % 2 == 0 else (False, True))
            got = device_call(ctx, plan, times, g_in, c_in, w, layout, *want)
            ref = host_call(plan, times, g_in, c_in, w, layout)
            for x, y in zip(got, ref):
                assert x is None or same_bits(y, x), (N, name, K, D, B, d, layout, j)
            if name == "standard" and j == 2:     # one case per N against the 50-digit reference (first two trajectories)
                gf, gx = [np.moveaxis(a, -1, 0) if layout == "soa" else a for a in got]
                r = R.reference(N, d, masks, times[:2], G[:2], c[:2], w)
                assert R.worst_share(gf[:2], r["free"], r["abs_free"], 3 * N + 12) <= 1.0
                assert R.worst_share(gx[:2], r["fixed"], r["abs_fixed"], 3 * N + 12) <= 1.0
                checked_reference = True
        # the Python method allocates what the raw call was handed: same bits
        pf, px = plan.free_gradient(*[torch.from_numpy(a).cuda() for a in (times, G, c)], 0.5, want_fixed=True)
        ctx.sync()
        hf, hx = host_call(plan, times, G, c, 0.5)
        assert same_bits(hf, pf.cpu().numpy()) and same_bits(hx, px.cpu().numpy())
        plan.close()
    assert checked_reference


@pytest.mark.parametrize("N,D,K,B", [(10, 16, 3, 9), (10, 17, 3, 9), (4, 40, 1, 3), (12, 16, 8, 5), (2, 16, 2, 70)])
def test_wide_dimensions(ctx, N, D, K, B):
    """D is a run-time value with no upper limit: widths at which a trajectory's (K + 1) D lanes straddle wavefronts and
    workgroups in other places than with D <= 4."""
    import mav_trajectory_generation_amd as m
    masks = pattern_masks("standard", N, K)
    plan = m.Plan(ctx, N, D, K, N // 2 - 1, masks)
    times, G, c = draw(N, K, D, B, 500 + D)
    for g_in, c_in in ((G, None), (None, c), (G, c)):
        got = device_call(ctx, plan, times, g_in, c_in, 0.5)
        ref = host_call(plan, times, g_in, c_in, 0.5)
        assert same_bits(ref[0], got[0]) and same_bits(ref[1], got[1]), (N, D, K, B)
    plan.close()


@pytest.mark.parametrize("N", [6, 10])
def test_adjoint_identity_against_update_from_free(ctx, N):
    """<J u, w> = <u, J^T w> with J u from Plan.update_from_free (d_fixed = 0) on the device."""
    import torch
    import mav_trajectory_generation_amd as m
    K, D, B = 3, 3, 5
    masks = pattern_masks("standard", N, K)
    plan = m.Plan(ctx, N, D, K, N // 2 - 1, masks)
    rng = np.random.default_rng(60 + N)
    times = rng.uniform(0.3, 4.0, (B, K))
    u = rng.standard_normal((B, D, plan.n_free))
    w = rng.standard_normal((B, K, D, N))
    t_d = torch.from_numpy(times).cuda()
    Ju, _ = plan.update_from_free(t_d, torch.zeros((B, D, plan.n_fixed), dtype=torch.float64, device="cuda"), torch.from_numpy(u).cuda())
    JTw, _ = plan.free_gradient(t_d, torch.from_numpy(w).cuda())
    ctx.sync()
    Ju, JTw = Ju.cpu().numpy(), JTw.cpu().numpy()
    ref = R.reference(N, plan.deriv, masks, times, w)
    for b in range(B):
        lhs, rhs = float(np.vdot(Ju[b], w[b])), float(np.vdot(u[b], JTw[b]))
        bound = (2 * N + 8) * E * float(sum(abs(x) * s for x, s in zip(u[b].ravel(), ref["abs_free"][b].ravel())))
        assert abs(lhs - rhs) <= 1e-9 * np.linalg.norm(Ju[b]) * np.linalg.norm(w[b]) + bound, (N, b, lhs, rhs)
    plan.close()


def test_special_times_follow_the_arithmetic_in_their_own_rows(ctx):
    import mav_trajectory_generation_amd as m
    N, K, D, B = 8, 3, 3, 6
    masks = pattern_masks("standard", N, K)
    plan = m.Plan(ctx, N, D, K, 2, masks)
    times, G, c = draw(N, K, D, B, 12)
    clean = device_call(ctx, plan, times, G, c, 1.0)
    bad = times.copy()
    bad[1, 1], bad[4, 0] = 0.0, np.nan
    got = device_call(ctx, plan, bad, G, c, 1.0)
    ref = host_call(plan, bad, G, c, 1.0)
    for x, y, z in zip(got, ref, clean):
        assert same_bits(y, x)
        assert same_bits(z[[0, 2, 3, 5]], x[[0, 2, 3, 5]])
        assert not np.isfinite(x[1]).all() and np.isnan(x[4]).any()
    plan.close()


def test_argument_table_with_a_real_plan(ctx):
    import torch
    import mav_trajectory_generation_amd as m
    N, K, D, B = 6, 2, 3, 2
    plan = m.Plan(ctx, N, D, K, 1, pattern_masks("standard", N, K))
    lay = plan.layout(B, "aos")
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    t, g, c, f, x = z(B, K) + 1.0, z(B, K, D, N), z(B, K, D, N), z(B, D, plan.n_free), z(B, D, plan.n_fixed)
    p = lambda a: ctypes.c_void_p(0) if a is None else ctypes.c_void_p(a.data_ptr())
    call = lambda batch, lay_, t_, g_, c_, f_, x_: ctx.lib.mtg_free_gradient(plan.handle, batch, lay_, p(t_), p(g_), p(c_), 1.0, p(f_), p(x_))
    L_ = ctypes.byref(lay)
    assert call(B, L_, t, g, c, f, x) == 0 and call(B, L_, t, g, None, f, None) == 0 and call(B, L_, t, None, c, None, x) == 0
    assert call(0, L_, t, g, c, f, x) == 0
    for args in ((-1, L_, t, g, c, f, x), (B, None, t, g, c, f, x), (B, L_, None, g, c, f, x), (B, L_, t, None, None, f, x),
                 (B, L_, t, g, c, None, None), (1 << 40, L_, t, g, c, f, x)):
        assert call(*args) == -1, args
    ctx.sync()
    plan.close()
