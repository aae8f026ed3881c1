"""Half-plane / flight-corridor feasibility check on the device (mtg_check_half_plane_feasibility, csrc/mtg_halfplane.hip):
against the reference's own candidates and evaluation (tests/golden/reference_half_plane_*.npz), against the library's host
build of the same lane code at the shapes where the kernel could go wrong, and captured into a graph."""
import numpy as np
import pytest

from test_half_plane import CASES, clearance_bound, load_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import mav_trajectory_generation_amd as m
    c = m.Context(0)
    yield c
    c.close()


def on_device(ctx, coeffs, times, planes, layout="aos", want_clearance=True):
    import torch
    import mav_trajectory_generation_amd as m
    t = times if layout == "aos" else np.ascontiguousarray(times.T)
    out = m.check_half_plane_feasibility(ctx, torch.from_numpy(np.ascontiguousarray(coeffs)).cuda(), torch.from_numpy(np.ascontiguousarray(t)).cuda(),
                                         torch.from_numpy(np.ascontiguousarray(planes)).cuda(), times_layout=layout,
                                         want_clearance=want_clearance)
    ctx.sync()
    return m.HalfPlaneFeasibilityResult(*[o.cpu().numpy() if o is not None else None for o in out])


def same_as_host(ctx, coeffs, times, planes, layout="aos"):
    """Device against host form: equal verdicts and indices, clearances within the project's bound; returns the device result."""
    import mav_trajectory_generation_amd as m
    h = m.check_half_plane_feasibility_host(coeffs, times, planes)
    d = on_device(ctx, coeffs, times, planes, layout)
    assert np.array_equal(d.trajectory_feasible, h.trajectory_feasible)
    assert np.array_equal(d.first_failing_segment, h.first_failing_segment)
    assert np.array_equal(d.first_failing_plane, h.first_failing_plane)
    bound = clearance_bound(coeffs, times, planes)
    err = np.abs(d.segment_clearance - h.segment_clearance)
    print(f"device vs host: max clearance difference {err.max():.2e}")
    assert (err <= bound).all()
    assert np.array_equal(d.trajectory_clearance, d.segment_clearance.min(axis=1))
    return d


@pytest.mark.parametrize("name", CASES)
def test_device_entry_vs_reference(ctx, name):
    """N = 10, 12 and the zero-padded 5 and 7; B x K = 300, 800 (B = 100, K = 8: 12.5 workgroups), 200 (K = 1), 240, 120, 160;
    D = 3 and 4; the shared plane set and (n10_k2_d3) a corridor per trajectory."""
    coeffs, times, z = load_case(name)
    for s in z["plane_sets"]:
        planes = z[f"{s}/planes"]
        d = on_device(ctx, coeffs, times, planes)
        assert np.array_equal(d.trajectory_feasible, z[f"{s}/trajectory_feasible"]), s
        assert np.array_equal(d.first_failing_segment, z[f"{s}/first_failing_segment"]), s
        assert np.array_equal(d.first_failing_plane, z[f"{s}/first_failing_plane"]), s
        err = np.abs(d.segment_clearance - z[f"{s}/segment_clearance"])
        print(f"{name}/{s}: max clearance error {err.max():.2e}")
        assert (err <= clearance_bound(coeffs, times, planes)).all(), s
        assert np.array_equal(d.trajectory_clearance, d.segment_clearance.min(axis=1))
    same_as_host(ctx, coeffs, times, z["oblique/planes"])


def test_one_segment_one_trajectory_and_n3(ctx):
    """B = 1, K = 1 (one lane of one workgroup) on the reference test's N = 3 parabola."""
    import mav_trajectory_generation_amd as m
    coeffs = np.zeros((1, 1, 3, 3))
    coeffs[0, 0, 0, 1] = 1.0
    coeffs[0, 0, 2, 2] = 1.0
    times = np.ones((1, 1))
    for zed, feasible in ((-0.2, 0), (-0.3, 1)):
        d = same_as_host(ctx, coeffs, times, m.half_planes([[0.0, 0.0, zed]], [[-1.0, 0.0, 1.0]]))   # P = 1
        assert int(d.trajectory_feasible[0]) == feasible and int(d.first_failing_plane[0]) == (-1 if feasible else 0)
        assert abs(d.trajectory_clearance[0] - (-0.25 - zed) / np.sqrt(2.0)) <= 1e-12


def test_yaw_garbage_times_soa_and_all_stride_forms(ctx):
    """D = 4 with the yaw coefficients overwritten (ignored, even NaN / huge), times as [K][B], planes as [P][4], [K][P][4] and
    [B][K][P][4]; B K = 240 is no multiple of 64."""
    import mav_trajectory_generation_amd as m
    coeffs, times, z = load_case("n12_k4_d4")
    coeffs = coeffs.copy()
    ref = on_device(ctx, coeffs, times, z["box16/planes"])
    coeffs[:, :, 3] = np.random.default_rng(5).standard_normal(coeffs[:, :, 3].shape) * 1e200
    coeffs[::3, :, 3, 2] = np.nan
    for layout in ("aos", "soa"):
        d = same_as_host(ctx, coeffs, times, z["box16/planes"], layout)
        assert np.array_equal(d.segment_clearance, ref.segment_clearance)
        assert np.array_equal(d.first_failing_plane, ref.first_failing_plane)
    bsz, k = times.shape
    per_seg = np.stack([m.bounding_box_half_planes([0, 0, 0], [e] * 3) for e in (26, 16, 22, 18)])            # [K][6][4]
    a = same_as_host(ctx, coeffs, times, per_seg, "soa")
    rng = np.random.default_rng(6)
    per_traj = np.stack([np.stack([m.bounding_box_half_planes(rng.uniform(-1, 1, 3), rng.uniform(14, 24, 3)) for _ in range(k)])
                         for _ in range(bsz)])                                                                # [B][K][6][4]
    b = same_as_host(ctx, coeffs, times, per_traj)
    assert 0 < int(a.trajectory_feasible.sum()) < bsz and 0 < int(b.trajectory_feasible.sum()) < bsz
    same_as_host(ctx, coeffs, times, np.broadcast_to(per_seg, (bsz,) + per_seg.shape).copy())
    assert np.array_equal(on_device(ctx, coeffs, times, np.broadcast_to(per_seg, (bsz,) + per_seg.shape).copy()).segment_clearance,
                          a.segment_clearance)


def test_sixty_four_planes_and_the_last_plane_of_the_last_segment(ctx):
    """P = 64: 63 planes far away in every direction, then one that only the end of the LAST segment of some trajectories
    crosses; and a trajectory failing in two segments is reported by the lower one."""
    import mav_trajectory_generation_amd as m
    coeffs, times, _ = load_case("n10_k8_d3_fast")
    bsz, k = times.shape
    rng = np.random.default_rng(7)
    nrm = rng.standard_normal((63, 3))
    nrm /= np.sqrt((nrm * nrm).sum(axis=1, keepdims=True))
    far = m.half_planes(-1000.0 * nrm, nrm)
    # the last segment's end position, x: a plane x < limit just below the largest of them
    x_end = np.array([np.polyval(coeffs[b, k - 1, 0, ::-1], times[b, k - 1]) for b in range(bsz)])
    order = np.argsort(x_end)
    limit = 0.5 * (x_end[order[-1]] + x_end[order[-2]])
    planes = np.concatenate([far, m.half_planes([[limit, 0.0, 0.0]], [[-1.0, 0.0, 0.0]])])
    assert planes.shape == (64, 4)
    per_seg = np.broadcast_to(planes, (k, 64, 4)).copy()
    per_seg[:k - 1, 63] = far[0]                        # only the last segment carries the deciding plane
    d = same_as_host(ctx, coeffs, times, per_seg)
    failing = np.flatnonzero(d.trajectory_feasible == 0)
    assert order[-1] in failing and failing.size < bsz
    assert (d.first_failing_segment[failing] == k - 1).all() and (d.first_failing_plane[failing] == 63).all()
    assert (d.first_failing_segment[d.trajectory_feasible == 1] == -1).all()
    # two failing segments: the lower one is reported, with ITS first failing plane
    box = m.bounding_box_half_planes([0, 0, 0], [20, 20, 20])
    d = same_as_host(ctx, coeffs, times, box)
    n_fail = (d.segment_clearance <= 0.0).sum(axis=1)
    assert (n_fail >= 2).sum() >= 10
    for b in np.flatnonzero(n_fail >= 2):
        assert d.first_failing_segment[b] == np.flatnonzero(d.segment_clearance[b] <= 0.0)[0]


def test_optional_outputs_null_and_empty_batch(ctx):
    import torch
    coeffs, times, z = load_case("n10_k2_d3")
    full = on_device(ctx, coeffs, times, z["oblique/planes"])
    bare = on_device(ctx, coeffs, times, z["oblique/planes"], want_clearance=False)
    assert bare.segment_clearance is None and bare.trajectory_clearance is None
    assert np.array_equal(bare.trajectory_feasible, full.trajectory_feasible)
    assert np.array_equal(bare.first_failing_plane, full.first_failing_plane)
    co, ti, pl = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (coeffs, times, z["oblique/planes"]))
    feas = torch.full((coeffs.shape[0],), -7, dtype=torch.int32, device="cuda")
    clear = torch.full((coeffs.shape[0],), -7.0, dtype=torch.float64, device="cuda")

    def call(batch, first_seg=None, first_plane=None, seg_c=None, traj_c=None, n_planes=2, ps_b=0):
        return ctx.lib.mtg_check_half_plane_feasibility(ctx.handle, 10, 2, 3, batch, co.data_ptr(), ti.data_ptr(), 2, 1, pl.data_ptr(), n_planes,
                                                        ps_b, 0, feas.data_ptr(), first_seg, first_plane, seg_c, traj_c)
    torch.cuda.synchronize()
    assert call(coeffs.shape[0], traj_c=clear.data_ptr()) == 0      # only the trajectory clearance: no per-segment table to reduce
    ctx.sync()
    assert np.array_equal(feas.cpu().numpy(), full.trajectory_feasible)
    assert np.array_equal(clear.cpu().numpy(), full.trajectory_clearance)
    feas.fill_(-7)
    torch.cuda.synchronize()
    assert call(0) == 0                                             # batch = 0: nothing enqueued, nothing written
    ctx.sync()
    assert (feas.cpu().numpy() == -7).all()
    assert call(coeffs.shape[0], n_planes=65) == -1 and call(coeffs.shape[0], ps_b=-8) == -1
    assert b"n_planes" in ctx.lib.mtg_last_error_string(ctx.handle)
    ctx.sync()
    assert (feas.cpu().numpy() == -7).all()


def test_capture_and_replay(ctx):
    """The call is three kernel launches on the context's stream: captured once, replayed on new coefficients."""
    import torch
    coeffs, times, z = load_case("n10_k8_d3_fast")
    planes = z["box22/planes"]
    bsz, k = times.shape
    co, ti, pl = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (coeffs, times, planes))
    feas = torch.zeros((bsz,), dtype=torch.int32, device="cuda")
    fseg, fplane = torch.zeros_like(feas), torch.zeros_like(feas)
    seg_c = torch.zeros((bsz, k), dtype=torch.float64, device="cuda")
    traj_c = torch.zeros((bsz,), dtype=torch.float64, device="cuda")

    def call():
        assert ctx.lib.mtg_check_half_plane_feasibility(ctx.handle, 10, k, 3, bsz, co.data_ptr(), ti.data_ptr(), k, 1, pl.data_ptr(), 6, 0, 0,
                                                        feas.data_ptr(), fseg.data_ptr(), fplane.data_ptr(), seg_c.data_ptr(),
                                                        traj_c.data_ptr()) == 0
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
    want_feas = z["box22/trajectory_feasible"][::-1]
    assert np.array_equal(feas.cpu().numpy(), want_feas) and 0 < int(want_feas.sum()) < bsz
    assert np.array_equal(fseg.cpu().numpy(), z["box22/first_failing_segment"][::-1])
    assert np.array_equal(fplane.cpu().numpy(), z["box22/first_failing_plane"][::-1])
    assert (np.abs(seg_c.cpu().numpy() - z["box22/segment_clearance"][::-1]) <= clearance_bound(coeffs, times, planes)[::-1]).all()
    assert np.array_equal(traj_c.cpu().numpy(), seg_c.cpu().numpy().min(axis=1))
