"""Analytic input-feasibility check on the device (mtg_check_input_feasibility, csrc/mtg_feasibility.hip): against the reference's
own verdicts (tests/golden/reference_feasibility_*.npz), against the library's host build of the same lane code at production
sizes, and composed with the other post-solve steps."""
import ctypes
import glob
import os

import numpy as np
import pytest

import helpers
from test_feasibility import compare_with_fixture, constraints_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "reference_feasibility_*.npz")))


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import mav_trajectory_generation_amd as m
    c = m.Context(0)
    yield c
    c.close()


def on_device(ctx, coeffs, times, constraints, layout="aos"):
    import torch
    import mav_trajectory_generation_amd as m
    t = times if layout == "aos" else np.ascontiguousarray(times.T)
    out = m.check_input_feasibility(ctx, torch.from_numpy(np.ascontiguousarray(coeffs)).cuda(), torch.from_numpy(t).cuda(), constraints,
                                    times_layout=layout)
    ctx.sync()
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[len("reference_feasibility_"):-4] for p in GOLDEN])
def test_device_entry_vs_reference(ctx, path):
    assert GOLDEN
    z = np.load(path)
    for s in z["limit_sets"]:
        c = constraints_of(z[f"{s}/limits"], z[f"{s}/min_section_time_s"])
        traj, first, seg, bounds = on_device(ctx, z["coeffs"], z["times"], c)
        compare_with_fixture(z, s, traj, first, seg, bounds)


def solved_on_device(ctx, n, k, dim, bsz, seed):
    import torch
    import mav_trajectory_generation_amd as m
    masks, times, d_fixed = helpers.reference_batch(bsz, k, n, dim, seed)
    plan = m.Plan(ctx, n, dim, k, n // 2 - 1, masks)
    t_dev = torch.from_numpy(times).cuda()
    coeffs, _, _ = plan.solve(t_dev, torch.from_numpy(d_fixed).cuda())
    ctx.sync()
    plan.close()
    return coeffs, t_dev


@pytest.mark.parametrize("n,k,dim,bsz,which", [(10, 8, 3, 10000, "defaults"), (10, 16, 4, 12500, "all_six")])
def test_device_vs_host_at_production_size(ctx, n, k, dim, bsz, which):
    import torch
    import mav_trajectory_generation_amd as m
    coeffs, t_dev = solved_on_device(ctx, n, k, dim, bsz, 4242)
    if which == "defaults":
        c = m.InputConstraints.defaults()
    else:
        c = m.InputConstraints(f_min=4.9, f_max=14.7, v_max=3.0, omega_xy_max=1.57, omega_z_max=1.57, omega_z_dot_max=6.28)
    co_h, t_h = coeffs.cpu().numpy(), t_dev.cpu().numpy()
    h_traj, h_first, h_seg, h_bounds = m.check_input_feasibility_host(co_h, t_h, c)
    d_traj, d_first, d_seg, d_bounds = [o.cpu().numpy() for o in m.check_input_feasibility(ctx, coeffs, t_dev, c)]
    ctx.sync()
    # bounds: within 1e-9 relative, NaN in the same places
    assert np.array_equal(np.isfinite(h_bounds), np.isfinite(d_bounds))
    ok = np.isfinite(h_bounds)
    rel = np.abs(d_bounds[ok] - h_bounds[ok]) / np.abs(h_bounds[ok])
    print(f"{which}: worst relative bound difference device vs host {rel.max():.2e}")
    assert (rel <= 1e-9).all()
    # verdicts: equal wherever no host bound lies within 1e-6 relative of the limit it is compared with
    limits = np.array([c.get_constraint(name) if c.has_constraint(name) else np.nan for name in
                       ("f_min", "f_max", "v_max", "omega_xy_max", "omega_z_max", "omega_z_dot_max")])
    marginal = np.zeros(h_seg.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        for q in range(6):
            lim = limits[q]
            if np.isfinite(lim):
                marginal |= np.abs(h_bounds[:, :, q] - lim) <= 1e-6 * lim
    clear = ~marginal.any(axis=1)
    share = 1.0 - clear.mean()
    print(f"{which}: verdict mix {dict(zip(*np.unique(h_traj, return_counts=True)))}, excluded share {share:.2e}")
    assert share <= 0.01
    assert np.array_equal(d_seg[clear], h_seg[clear])
    assert np.array_equal(d_traj[clear], h_traj[clear]) and np.array_equal(d_first[clear], h_first[clear])
    assert (d_seg != 5).all()
    # the same batch with [K][B] times: bit-identical outputs
    soa = m.check_input_feasibility(ctx, coeffs, t_dev.t().contiguous(), c, times_layout="soa")
    ctx.sync()
    for a, b in zip((d_traj, d_first, d_seg), soa[:3]):
        assert np.array_equal(a, b.cpu().numpy())
    assert np.array_equal(d_bounds, soa[3].cpu().numpy(), equal_nan=True)
    # the optional outputs are optional
    t_only, f_only, none_seg, none_bounds = m.check_input_feasibility(ctx, coeffs, t_dev, c, want_segments=False, want_bounds=False)
    ctx.sync()
    assert none_seg is None and none_bounds is None
    assert np.array_equal(t_only.cpu().numpy(), d_traj) and np.array_equal(f_only.cpu().numpy(), d_first)


def test_post_solve_steps_compose_on_the_device(ctx):
    """solve -> scale_segment_times_to_meet_constraints(v_max, a_max) -> check_input_feasibility with only a velocity limit of
    v_max (1 + 2e-3) (the scaling accepts an excess of 1e-3 relative, the check is a strict >): every within_range trajectory is
    feasible, without a host copy in between."""
    import mav_trajectory_generation_amd as m
    v_max, a_max = 2.0, 3.0
    coeffs, t_dev = solved_on_device(ctx, 10, 8, 3, 2000, 777)
    before = m.check_input_feasibility(ctx, coeffs, t_dev, m.InputConstraints(v_max=v_max * (1 + 2e-3)))[0]
    _, within, _ = m.scale_segment_times_to_meet_constraints(ctx, coeffs, t_dev, v_max, a_max)
    after = m.check_input_feasibility(ctx, coeffs, t_dev, m.InputConstraints(v_max=v_max * (1 + 2e-3)))[0]
    ctx.sync()
    before, within, after = before.cpu().numpy(), within.cpu().numpy(), after.cpu().numpy()
    assert within.sum() > 1000 and (before == 4).sum() > 100        # the scaling had something to do
    assert (after[within == 1] == 0).all()
    assert set(np.unique(after)) <= {0, 4}


def test_argument_errors_enqueue_nothing(ctx):
    import torch
    import mav_trajectory_generation_amd as m
    co = torch.zeros((2, 3, 3, 10), dtype=torch.float64, device="cuda")
    ti = torch.ones((2, 3), dtype=torch.float64, device="cuda")
    traj = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    c = m.InputConstraints.defaults().to_c()

    def call(n=10, k=3, d=3, b=2, coeffs=co.data_ptr(), times=ti.data_ptr(), sb=3, sk=1, cons=ctypes.byref(c), out=traj.data_ptr(), bounds=None):
        return ctx.lib.mtg_check_input_feasibility(ctx.handle, n, k, d, b, coeffs, times, sb, sk, cons, out, None, None, bounds)

    for bad in (dict(n=4), dict(n=13), dict(k=0), dict(d=0), dict(b=-1), dict(coeffs=None), dict(times=None), dict(cons=None),
                dict(out=None), dict(sb=0), dict(sk=-1), dict(sb=2, sk=1), dict(bounds=8)):
        assert call(**bad) == -1, bad
    assert call(n=13) == -1 and b"n_coeffs must be in [5,12]" in ctx.lib.mtg_last_error_string(ctx.handle)
    assert call(bounds=8) == -1 and b"16-byte aligned" in ctx.lib.mtg_last_error_string(ctx.handle)
    ctx.sync()
    assert (traj.cpu().numpy() == -7).all()                         # nothing ran
    assert call(b=0) == 0
    assert call() == 0
    ctx.sync()
    assert (traj.cpu().numpy() == 0).all()                          # hover: feasible under the default limits
    with pytest.raises(m.MtgError):
        m.check_input_feasibility(ctx, torch.zeros((1, 1, 3, 4), dtype=torch.float64, device="cuda"), ti[:1, :1].contiguous(), m.InputConstraints())
