"""The frame the per-segment root-search kernels share (csrc/mtg_segment_kernel.h, csrc/mtg_segment_lane.h): the lane index ->
(trajectory, segment, time, coefficients) code and the even-instantiation dispatch, under the four entries that use them --
mtg_check_input_feasibility, mtg_magnitude_soft_cost, mtg_check_half_plane_feasibility and mtg_minmax_magnitude.

  * lane counts around the workgroup edges: B x K = 63, 64, 65 and 43 x 3 = 129 for the 64-lane kernels; 127, 129 and 43 x 3 for the
    128-lane extrema kernel at one, two and four lanes per search; one case of each entry with [K][B] times;
  * every accepted coefficient count at B x K = 5 x 3: 5 .. 12 (feasibility), 1 .. 12 (half-plane), 4 .. 12 at D = 3 and 4 (objective);
  * every trajectory and segment distinct, so a slipped index shows: amplitudes, frequencies, phases and times are drawn per segment.

Each device result is compared with the host form of the same lane code (the extrema kernel: tests/extrema_emu.cpp): verdicts, first
failing segment and plane equal, values within 1e-9 relative (of the quantity, or for signed clearances and extrema of their
segment's scale, as in the entries' own GPU tests).  So that no verdict hinges on the last bits, every host bound and clearance
is asserted to lie at least 1e-6 relative away from its limit BEFORE anything is compared; test_host_values_keep_their_margins
asserts the same for all cases without a device."""
import functools
import math

import numpy as np
import pytest

import mav_trajectory_generation_amd as m
from objective_ref import order_groups
from test_extrema import xemu  # noqa: F401  (the fixture: tests/libmtg_extrema_emu.so)
from test_half_plane import clearance_bound

REL = 1e-9        # device against host, as in test_gpu_feasibility.py / test_gpu_half_plane.py / test_gpu_time_objective.py
MARGIN = 1e-6     # host bound or clearance against its limit
EDGES_64 = [(63, 1), (64, 1), (65, 1), (43, 3)]
EDGES_128 = [(127, 1), (129, 1), (43, 3)]
PER_N = (5, 3)

# (B, K, D, N, times layout)
FEASIBILITY = [(b, k, 4, 10, "aos") for b, k in EDGES_64] + [(43, 3, 4, 10, "soa")] + [PER_N + (4, n, "aos") for n in range(5, 13)]
OBJECTIVE = ([(b, k, 3, 10, "aos") for b, k in EDGES_64] + [(43, 3, 3, 10, "soa")] +
             [PER_N + (d, n, "aos") for d in (3, 4) for n in range(4, 13)])
HALF_PLANE = [(b, k, 3, 10, "aos") for b, k in EDGES_64] + [(43, 3, 3, 10, "soa")] + [PER_N + (3, n, "aos") for n in range(1, 13)]
EXTREMA = [(b, k, 3, 10, "aos", split) for b, k in EDGES_128 for split in (1, 2, 3)] + [(43, 3, 3, 10, "soa", 0)]   # 3: four lanes
ident = lambda c: "-".join(str(x) for x in c)


def inputs(bsz, k, d, n):
    """coeffs [B][K][D][N], times [B][K]: per segment and dimension the Taylor coefficients of A sin(w t + phase), A in [0.5, 2],
    w in [0.8, 2], T in [0.5, 2] -- every derivative oscillates (interior critical points), none is badly conditioned."""
    rng = np.random.default_rng(77000000 + 10000 * bsz + 1000 * k + 100 * d + n)
    times = rng.uniform(0.5, 2.0, size=(bsz, k))
    amp = rng.uniform(0.5, 2.0, size=(bsz, k, d, 1))
    w = rng.uniform(0.8, 2.0, size=(bsz, k, d, 1))
    phase = rng.uniform(0.0, 2.0 * math.pi, size=(bsz, k, d, 1))
    i = np.arange(n, dtype=np.float64)
    fact = np.array([math.factorial(j) for j in range(n)], dtype=np.float64)
    return np.ascontiguousarray(amp * w ** i * np.sin(phase + i * (math.pi / 2.0)) / fact), times


def laid_out(times, layout):
    return times if layout == "aos" else np.ascontiguousarray(times.T)


def away_from(values, limit, scale=None):
    """Every finite value at least MARGIN (relative to the limit, or to `scale`) away from its limit."""
    values = np.asarray(values, dtype=np.float64)
    ok = np.isfinite(values)
    gap = np.abs(values - limit)
    need = MARGIN * (np.abs(limit) if scale is None else scale)
    return bool((gap[ok] >= np.broadcast_to(need, values.shape)[ok]).all())


# ---- input feasibility ----------------------------------------------------------------------------------------------------------
LIMITS = dict(f_min=5.0, f_max=14.0, v_max=3.4, omega_xy_max=0.8, omega_z_max=3.0, omega_z_dot_max=5.0)


@functools.lru_cache(maxsize=None)
def feasibility_host(case):
    bsz, k, d, n, layout = case
    coeffs, times = inputs(bsz, k, d, n)
    con = m.InputConstraints(**LIMITS)
    traj, first, seg, bounds = m.check_input_feasibility_host(coeffs, laid_out(times, layout), con, times_layout=layout)
    for q, name in enumerate(m.InputConstraints.NAMES):      # (the columns of segment_bounds are in the order of NAMES)
        assert away_from(bounds[:, :, q], LIMITS[name]), (case, name)
    return coeffs, times, con, traj, first, seg, bounds


# ---- time objective: maxima + soft cost ---------------------------------------------------------------------------------------------
def objective_params(group):
    # (weight 1: a soft term is exp((max - limit) / limit), as well conditioned as the maximum itself)
    return m.TimeObjectiveParams(soft_constraint_weight=1.0, constraints=[(der, 1.0 + der) for der in group])


@functools.lru_cache(maxsize=None)
def objective_host(case):
    bsz, k, d, n, layout = case
    coeffs, times = inputs(bsz, k, d, n)
    out = [m.magnitude_soft_cost_host(coeffs, laid_out(times, layout), objective_params(g), times_layout=layout) for g in order_groups(n)]
    return coeffs, times, out


# ---- half planes ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def half_plane_host(case):
    bsz, k, d, n, layout = case
    coeffs, times = inputs(bsz, k, d, n)
    planes = m.bounding_box_half_planes([0.1, -0.1, 0.0], [2.6, 2.8, 3.0])
    res = m.check_half_plane_feasibility_host(coeffs, laid_out(times, layout), planes, times_layout=layout)
    scale = clearance_bound(coeffs, times, planes) / 1e-9                  # max(1, |offset| + max |p| over the segment), [B][K]
    for h in range(planes.shape[0]):                                        # plane by plane: the first failing PLANE must not hinge either
        one = m.check_half_plane_feasibility_host(coeffs, laid_out(times, layout), planes[h:h + 1], times_layout=layout)
        assert away_from(one.segment_clearance, 0.0, scale), (case, h)
    return coeffs, times, planes, res


# ---- magnitude extrema ------------------------------------------------------------------------------------------------------------
def extrema_host(lib, case, derivative):
    bsz, k, d, n = case[:4]
    coeffs, times = inputs(bsz, k, d, n)
    out = np.zeros((bsz, k, 4))
    assert lib.extrema_emu_segments(n, k, d, bsz, coeffs.ctypes.data, times.ctypes.data, derivative, (1 << d) - 1, out.ctypes.data) == 0
    return coeffs, times, out


def test_host_values_keep_their_margins():
    """Every case's host values are MARGIN away from their limits (the seeds were chosen on the host for that), and the verdicts
    are mixed: the comparisons of first failing segments and planes below compare something."""
    codes, planes_seen = set(), set()
    for case in FEASIBILITY:
        _, _, _, traj, first, seg, _ = feasibility_host(case)
        codes |= set(int(c) for c in np.unique(seg))
        if case[:2] == (43, 3):
            assert (first > 0).any() and (traj == 0).any()
    assert {0, 1, 2, 3, 4, 6, 7} <= codes, codes
    for case in HALF_PLANE:
        res = half_plane_host(case)[3]
        planes_seen |= set(int(p) for p in res.first_failing_plane)
        if case[:2] == (43, 3):
            assert (res.first_failing_segment > 0).any() and (res.trajectory_feasible == 1).any()
    assert len(planes_seen - {-1}) >= 4, planes_seen


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = m.Context(0)
    yield c
    c.close()


def to_device(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


@pytest.mark.gpu
@pytest.mark.parametrize("case", FEASIBILITY, ids=ident)
def test_feasibility_device_vs_host(ctx, case):
    coeffs, times, con, traj, first, seg, bounds = feasibility_host(case)
    co, tt = to_device(coeffs, laid_out(times, case[4]))
    d_traj, d_first, d_seg, d_bounds = (o.cpu().numpy() for o in m.check_input_feasibility(ctx, co, tt, con, times_layout=case[4]))
    assert np.array_equal(d_seg, seg) and np.array_equal(d_traj, traj) and np.array_equal(d_first, first)
    assert np.array_equal(np.isnan(d_bounds), np.isnan(bounds))
    wrote = ~np.isnan(bounds)
    rel = np.abs(d_bounds[wrote] - bounds[wrote]) / np.abs(bounds[wrote])
    print(f"feasibility {ident(case)}: worst relative bound difference {rel.max():.2e}")
    assert (rel <= REL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", OBJECTIVE, ids=ident)
def test_objective_device_vs_host(ctx, case):
    coeffs, times, host = objective_host(case)
    co, tt = to_device(coeffs, laid_out(times, case[4]))
    for group, (h_cost, h_max, h_vio) in zip(order_groups(case[3]), host):
        p = objective_params(group)
        cost, maxima, vio = (o.cpu().numpy() for o in m.magnitude_soft_cost(ctx, co, tt, p, times_layout=case[4]))
        rel = np.abs(maxima - h_max) / h_max
        print(f"objective {ident(case)} orders {group}: worst relative difference of a maximum {rel.max():.2e}")
        assert (rel <= REL).all()
        limits = np.array([v for _, v in p.constraints])
        assert np.array_equal(vio, maxima - limits)
        # a term exp((max - limit) / limit) moves by (max / limit) times the maximum's relative difference
        assert (np.abs(cost - h_cost) <= (REL * (1.0 + (h_max / limits).max(axis=1)) + 8 * np.finfo(np.float64).eps) * h_cost).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", HALF_PLANE, ids=ident)
def test_half_plane_device_vs_host(ctx, case):
    coeffs, times, planes, h = half_plane_host(case)
    co, tt, pl = to_device(coeffs, laid_out(times, case[4]), planes)
    d = m.HalfPlaneFeasibilityResult(*[o.cpu().numpy() for o in m.check_half_plane_feasibility(ctx, co, tt, pl, times_layout=case[4])])
    assert np.array_equal(d.trajectory_feasible, h.trajectory_feasible)
    assert np.array_equal(d.first_failing_segment, h.first_failing_segment)
    assert np.array_equal(d.first_failing_plane, h.first_failing_plane)
    err = np.abs(d.segment_clearance - h.segment_clearance)
    print(f"half-plane {ident(case)}: largest clearance difference {err.max():.2e}")
    assert (err <= clearance_bound(coeffs, times, planes)).all()
    assert np.array_equal(d.trajectory_clearance, d.segment_clearance.min(axis=1))


@pytest.mark.gpu
@pytest.mark.parametrize("case", EXTREMA, ids=ident)
def test_extrema_device_vs_host(ctx, xemu, case):  # noqa: F811
    layout, split = case[4], case[5]
    try:
        ctx.set_option("extrema_split", split)      # (bits 0-1: lanes per search: 1, 2, 3 = four; 0 = by launch size)
        for derivative in (1, 2):
            coeffs, times, want = extrema_host(xemu, case, derivative)
            co, tt = to_device(coeffs, laid_out(times, layout))
            seg, traj, idx = (o.cpu().numpy() for o in m.minmax_magnitude(ctx, co, tt, derivative, times_layout=layout))
            scale = np.abs(want[:, :, 3]).max(axis=1, keepdims=True)      # per trajectory
            err = np.abs(seg[:, :, [1, 3]] - want[:, :, [1, 3]]) / scale[:, :, None]
            print(f"extrema {ident(case)} derivative {derivative}: worst difference of an extremum {err.max():.2e} of its trajectory's maximum")
            assert (err <= REL).all()
            # the trajectory fold on the device's own table: the first segment with a strictly smaller / larger value
            k_min, k_max = seg[:, :, 1].argmin(axis=1), seg[:, :, 3].argmax(axis=1)
            rows = np.arange(seg.shape[0])
            assert np.array_equal(idx, np.stack([k_min, k_max], axis=1))
            assert np.array_equal(traj[:, :2], seg[rows, k_min, :2]) and np.array_equal(traj[:, 2:], seg[rows, k_max, 2:])
    finally:
        ctx.set_option("extrema_split", -1)
