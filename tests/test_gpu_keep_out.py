"""Keep-out zone check on the device (mtg_check_keep_out_zones, csrc/mtg_keepout.hip): against the reference's own root finders
and evaluation (tests/golden/reference_keep_out_*.npz), against the independent longdouble reference (tests/keep_out_ref.py),
against the library's host build of the same lane code at the shapes where the kernel could go wrong, and captured into a graph."""
import numpy as np
import pytest

import keep_out_ref as R
from test_keep_out import CASES, check_against_fixture, compare_with_independent_reference, fixture_scale, load_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import mav_trajectory_generation_amd as m
    c = m.Context(0)
    yield c
    c.close()


def on_device(ctx, coeffs, times, zones, inflation=0.0, layout="aos", want_clearance=True):
    import torch
    import mav_trajectory_generation_amd as m
    t = times if layout == "aos" else np.ascontiguousarray(times.T)
    out = m.check_keep_out_zones(ctx, torch.from_numpy(np.array(coeffs)).cuda(), torch.from_numpy(np.array(t)).cuda(),
                                 torch.from_numpy(np.array(zones)).cuda(), inflation=inflation, times_layout=layout,
                                 want_clearance=want_clearance)
    ctx.sync()
    return m.KeepOutResult(*[o.cpu().numpy() if o is not None else None for o in out])


def same_as_host(ctx, coeffs, times, zones, inflation=0.0, layout="aos"):
    """Device against host form: verdicts and indices bit for bit, clearances within 1e-9 max(1, scale); returns the device result."""
    import mav_trajectory_generation_amd as m
    h = m.check_keep_out_zones_host(coeffs, times, zones, inflation=inflation)
    d = on_device(ctx, coeffs, times, zones, inflation, layout)
    assert np.array_equal(d.trajectory_feasible, h.trajectory_feasible)
    assert np.array_equal(d.first_failing_segment, h.first_failing_segment)
    assert np.array_equal(d.first_failing_zone, h.first_failing_zone)
    assert np.array_equal(d.segment_nearest_zone, h.segment_nearest_zone)
    bound = 1e-9 * np.maximum(1.0, R.scale_of(coeffs, times, zones, inflation).max(axis=1))[:, None]
    err = np.abs(d.segment_clearance - h.segment_clearance)
    print(f"device vs host: max clearance difference {err.max():.2e}, largest share of the bound {(err / bound).max():.2e}")
    assert (err <= bound).all()
    assert np.array_equal(d.trajectory_clearance, d.segment_clearance.min(axis=1))
    return d


@pytest.mark.parametrize("name", CASES)
def test_device_entry_vs_reference(ctx, name):
    """N = 10, 12 and the zero-padded 5 and 7; B x K = 300, 800 (12.5 workgroups), 200 (K = 1), 240, 120, 160; D = 3 and 4;
    M = 16 and 1, shared, and (n10_k2_d3) four boxes per trajectory."""
    check_against_fixture(name, lambda c, t, z, infl: on_device(ctx, c, t, z, infl))
    coeffs, times, z = load_case(name)
    same_as_host(ctx, coeffs, times, z["z16_inflated/zones"], 0.3)
    if name == "n10_k2_d3":
        same_as_host(ctx, coeffs, times, z["per_trajectory/zones"])


@pytest.mark.parametrize("n,d,family", R.CASES, ids=[f"n{n}_d{d}_{f}" for n, d, f in R.CASES])
def test_every_instantiation_at_65_segments(ctx, n, d, family):
    """13 x 5 segments: one full workgroup plus one lane, in the instantiations 4, 6, 8, 10, 12 (odd N zero-padded)."""
    z = R.reference(n, d, family)
    r = on_device(ctx, z["coeffs"], z["times"], z["zones"])
    compare_with_independent_reference(n, d, family, r)
    same_as_host(ctx, z["coeffs"], z["times"], z["zones"])


@pytest.mark.parametrize("n_zones", [1, 2, 16, 300])
def test_zone_counts_shared_and_per_trajectory(ctx, n_zones):
    """M = 1, 2, 16 and 300 (nothing is staged, so no size is special: 300 is several times a wavefront), as one shared set and
    as a set per trajectory; times as [K][B] for the second."""
    z = R.reference(10, 3, "through")
    rng = np.random.default_rng(300 + n_zones)
    base = z["zones"]
    if n_zones <= len(base):
        zones = base[:n_zones].copy()
    else:   # the curve's own boxes scattered among far ones (moved along a plane's normal by s: its offset grows by n . s)
        reps = -(-n_zones // len(base))
        zones = np.tile(base, (reps, 1, 1))[:n_zones].copy()
        far = rng.permutation(n_zones)[: n_zones - len(base)]
        shift = rng.uniform(20.0, 60.0, (far.size, 3)) * rng.choice([-1.0, 1.0], (far.size, 3))
        zones[far, :, 3] += (zones[far, :, :3] * shift[:, None, :]).sum(axis=2)
    same_as_host(ctx, z["coeffs"], z["times"], zones)
    per = np.stack([zones[rng.permutation(n_zones)] for _ in range(R.B)])
    shift = rng.uniform(-0.5, 0.5, (R.B, 1, 1, 3))
    per[..., 3] += (per[..., :3] * shift).sum(axis=-1)
    same_as_host(ctx, z["coeffs"], z["times"], per, layout="soa")


@pytest.mark.parametrize("planes", [1, 4, 8])
def test_planes_per_zone(ctx, planes):
    """P = 1, 4 and 8 (6 is every other test): the box's first planes, and the box padded with two repeated planes."""
    z = R.reference(9, 4, "corner")
    zones = z["zones"][:, :planes] if planes <= 6 else np.concatenate([z["zones"], z["zones"][:, 1:3]], axis=1)
    d = same_as_host(ctx, z["coeffs"], z["times"], np.ascontiguousarray(zones))
    if planes == 8:
        assert all(np.array_equal(a, b) for a, b in zip(d, on_device(ctx, z["coeffs"], z["times"], z["zones"])))


def test_yaw_is_never_read_and_nan_wins(ctx):
    coeffs, times, z = load_case("n12_k4_d4")
    zones = z["z16/zones"]
    clean = on_device(ctx, coeffs, times, zones)
    dirty = coeffs.copy()
    dirty[:, :, 3] = np.nan
    assert all(np.array_equal(a, b) for a, b in zip(on_device(ctx, dirty, times, zones), clean))
    dirty = coeffs.copy()
    dirty[7, 2, 0, 3] = np.nan
    d = on_device(ctx, dirty, times, zones)
    assert d.trajectory_feasible[7] == 0 and np.isnan(d.segment_clearance[7, 2]) and np.isnan(d.trajectory_clearance[7])
    assert d.segment_nearest_zone[7, 2] == 0
    others = np.arange(len(coeffs)) != 7
    for a, b in zip(d, clean):
        assert np.array_equal(a[others], b[others])
    bad = zones.copy()     # (the device entry does not verify the planes)
    bad[9, 2, 3] = np.nan
    d = on_device(ctx, coeffs, times, bad)
    assert not d.trajectory_feasible.any() and (d.first_failing_segment == 0).all() and (d.segment_nearest_zone == 9).all()
    assert np.isnan(d.segment_clearance).all() and np.isnan(d.trajectory_clearance).all()
    # segment times that are not positive: the ends only, as on the host
    import mav_trajectory_generation_amd as m
    t_bad = times.copy()
    t_bad[1, 0], t_bad[2, 1] = 0.0, -0.5
    d, h = on_device(ctx, coeffs, t_bad, zones), m.check_keep_out_zones_host(coeffs, t_bad, zones)
    assert np.array_equal(d.trajectory_feasible, h.trajectory_feasible) and np.array_equal(d.segment_closest_time[[1, 2], [0, 1]], h.segment_closest_time[[1, 2], [0, 1]])
    assert np.abs(d.segment_clearance - h.segment_clearance).max() <= 1e-9 * 30.0


def test_optional_outputs_null_empty_batch_and_argument_errors(ctx):
    import torch
    coeffs, times, z = load_case("n10_k2_d3")
    zones = z["z16/zones"]
    full = on_device(ctx, coeffs, times, zones)
    bare = on_device(ctx, coeffs, times, zones, want_clearance=False)
    assert bare.segment_clearance is None and bare.trajectory_clearance is None
    assert np.array_equal(bare.trajectory_feasible, full.trajectory_feasible)
    assert np.array_equal(bare.first_failing_zone, full.first_failing_zone)
    co, ti, zo = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (coeffs, times, zones))
    bsz = coeffs.shape[0]
    feas = torch.full((bsz,), -7, dtype=torch.int32, device="cuda")
    clear = torch.full((bsz,), -7.0, dtype=torch.float64, device="cuda")

    def call(batch, traj_c=None, n_zones=16, n_planes=6, zs_b=0, inflation=0.0, dim=3, k=2):
        return ctx.lib.mtg_check_keep_out_zones(ctx.handle, 10, k, dim, batch, co.data_ptr(), ti.data_ptr(), 2, 1, zo.data_ptr(), n_zones,
                                                n_planes, zs_b, inflation, feas.data_ptr(), None, None, None, None, None, traj_c)
    torch.cuda.synchronize()
    assert call(bsz, traj_c=clear.data_ptr()) == 0      # only the trajectory clearance: no per-segment table to reduce
    ctx.sync()
    assert np.array_equal(feas.cpu().numpy(), full.trajectory_feasible)
    assert np.array_equal(clear.cpu().numpy(), full.trajectory_clearance)
    feas.fill_(-7)
    torch.cuda.synchronize()
    assert call(0) == 0                                 # batch = 0: nothing enqueued, nothing written
    for bad in (dict(n_zones=0), dict(n_zones=4097), dict(n_planes=0), dict(n_planes=9), dict(zs_b=-4), dict(inflation=-0.1),
                dict(inflation=float("nan")), dict(inflation=float("inf")), dict(dim=2), dict(dim=5), dict(k=1 << 19)):
        assert call(bsz, **bad) == -1, bad
        assert b"keep-out zones" in ctx.lib.mtg_last_error_string(ctx.handle)
    ctx.sync()
    assert (feas.cpu().numpy() == -7).all()


def test_capture_and_replay(ctx):
    """The call is three kernel launches on the context's stream, a linear chain: captured once, replayed once on new coefficients."""
    import torch
    coeffs, times, z = load_case("n10_k8_d3_fast")
    zones = z["z16/zones"]
    bsz, k = times.shape
    co, ti, zo = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (coeffs, times, zones))
    feas = torch.zeros((bsz,), dtype=torch.int32, device="cuda")
    fseg, fzone = torch.zeros_like(feas), torch.zeros_like(feas)
    seg_c = torch.zeros((bsz, k), dtype=torch.float64, device="cuda")
    seg_z = torch.zeros((bsz, k), dtype=torch.int32, device="cuda")
    seg_t = torch.zeros_like(seg_c)
    traj_c = torch.zeros((bsz,), dtype=torch.float64, device="cuda")

    def call():
        assert ctx.lib.mtg_check_keep_out_zones(ctx.handle, 10, k, 3, bsz, co.data_ptr(), ti.data_ptr(), k, 1, zo.data_ptr(), 16, 6, 0, 0.0,
                                                feas.data_ptr(), fseg.data_ptr(), fzone.data_ptr(), seg_c.data_ptr(), seg_z.data_ptr(),
                                                seg_t.data_ptr(), traj_c.data_ptr()) == 0
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
    g.replay()
    torch.cuda.synchronize()
    want_feas = z["z16/trajectory_feasible"][::-1]
    assert np.array_equal(feas.cpu().numpy(), want_feas) and 0 < int(want_feas.sum()) < bsz
    assert np.array_equal(fseg.cpu().numpy(), z["z16/first_failing_segment"][::-1])
    assert np.array_equal(fzone.cpu().numpy(), z["z16/first_failing_zone"][::-1])
    scale = fixture_scale(z, "z16").max(axis=1)[::-1, None]
    assert (np.abs(seg_c.cpu().numpy() - z["z16/segment_clearance"][::-1]) <= 1e-6 * scale).all()
    assert np.array_equal(traj_c.cpu().numpy(), seg_c.cpu().numpy().min(axis=1))
