"""Recursive input-feasibility check on the device (mtg_check_input_feasibility_recursive, csrc/mtg_recursive.hip): against the
reference's verdicts, bounds and section counts (tests/golden/reference_recursive_feasibility_*.npz) on every case -- N = 7, 10
and 12, D = 3 and 4, K = 1, 2, 4 and 8, B = 40 .. 200, lane counts that are no multiple of the 64-lane workgroup -- and bit for
bit against the library's host build of the same lane code."""
import ctypes

import numpy as np
import pytest

from test_recursive_feasibility import GOLDEN, IDS, compare_with_fixture, constraints_of, load_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import mav_trajectory_generation_amd as m
    c = m.Context(0)
    yield c
    c.close()


def on_device(ctx, coeffs, times, constraints, layout="aos", **want):
    import torch
    import mav_trajectory_generation_amd as m
    t = times if layout == "aos" else np.ascontiguousarray(times.T)
    out = m.check_input_feasibility_recursive(ctx, torch.from_numpy(np.ascontiguousarray(coeffs)).cuda(), torch.from_numpy(t).cuda(),
                                              constraints, times_layout=layout, **want)
    ctx.sync()
    return [o if o is None else o.cpu().numpy() for o in out]


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_device_entry_vs_reference_and_host(ctx, path):
    import mav_trajectory_generation_amd as m
    assert len(GOLDEN) == 7
    z, coeffs, times = load_case(path)
    assert (coeffs.shape[0] * coeffs.shape[1]) % 64 != 0            # the last workgroup is partial
    for s in z["limit_sets"]:
        c = constraints_of(z[f"{s}/limits"], z[f"{s}/min_section_time_s"])
        dev = on_device(ctx, coeffs, times, c, want_sections=True)
        compare_with_fixture(z, s, *dev)
        # the host build of the same lane code: verdicts and section counts bit for bit, on every trajectory
        host = m.check_input_feasibility_recursive_host(coeffs, times, c)
        for q in (0, 1, 2, 4):
            assert np.array_equal(dev[q], host[q]), (s, q)
        assert np.array_equal(np.isfinite(dev[3]), np.isfinite(host[3]))


def test_soa_times_and_optional_outputs(ctx):
    z, coeffs, times = load_case(GOLDEN[IDS.index("n10_k8_d3_fast")])
    c = constraints_of(z["no_velocity/limits"], z["no_velocity/min_section_time_s"])
    aos = on_device(ctx, coeffs, times, c, want_sections=True)
    soa = on_device(ctx, coeffs, times, c, layout="soa", want_sections=True)
    for a, b in zip(aos, soa):
        assert np.array_equal(a, b, equal_nan=True)
    # the optional outputs given as null pointers
    only = on_device(ctx, coeffs, times, c, want_segments=False, want_bounds=False)
    assert only[2] is None and only[3] is None and only[4] is None
    assert np.array_equal(only[0], aos[0]) and np.array_equal(only[1], aos[1])
    import torch
    co, ti = torch.from_numpy(coeffs).cuda(), torch.from_numpy(times).cuda()
    traj = torch.full((coeffs.shape[0],), -7, dtype=torch.int32, device="cuda")
    cc = c.to_c()
    bsz, k, dim, n = coeffs.shape
    assert ctx.lib.mtg_check_input_feasibility_recursive(ctx.handle, n, k, dim, bsz, co.data_ptr(), ti.data_ptr(), k, 1, ctypes.byref(cc),
                                                         traj.data_ptr(), None, None, None, None) == 0
    ctx.sync()
    assert np.array_equal(traj.cpu().numpy(), aos[0])


def test_captured_graph_replay_equals_the_direct_call(ctx):
    """The call is three kernel launches on the context's stream: captured once, replayed on new coefficients."""
    import torch
    z, coeffs, times = load_case(GOLDEN[IDS.index("n12_k4_d4")])
    c = constraints_of(z["all_six/limits"], z["all_six/min_section_time_s"])
    direct = on_device(ctx, coeffs[::-1], np.ascontiguousarray(times[::-1]), c, want_sections=True)
    bsz, k, dim, n = coeffs.shape
    co, ti = torch.from_numpy(coeffs).cuda(), torch.from_numpy(times).cuda()
    traj = torch.zeros((bsz,), dtype=torch.int32, device="cuda")
    first = torch.zeros_like(traj)
    seg = torch.zeros((bsz, k), dtype=torch.int32, device="cuda")
    sections = torch.zeros_like(seg)
    bounds = torch.zeros((bsz, k, 6), dtype=torch.float64, device="cuda")
    cc = c.to_c()

    def call():
        assert ctx.lib.mtg_check_input_feasibility_recursive(ctx.handle, n, k, dim, bsz, co.data_ptr(), ti.data_ptr(), k, 1, ctypes.byref(cc),
                                                             traj.data_ptr(), first.data_ptr(), seg.data_ptr(), bounds.data_ptr(),
                                                             sections.data_ptr()) == 0
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
    for a, b in zip(direct, (traj, first, seg, bounds, sections)):
        assert np.array_equal(a, b.cpu().numpy(), equal_nan=True)
    assert len(np.unique(direct[0])) >= 3


def test_argument_errors_and_empty_batch_enqueue_nothing(ctx):
    import torch
    import mav_trajectory_generation_amd as m
    co = torch.zeros((2, 3, 3, 10), dtype=torch.float64, device="cuda")
    ti = torch.ones((2, 3), dtype=torch.float64, device="cuda")
    traj = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    c = m.InputConstraints.defaults().to_c()

    def call(n=10, k=3, d=3, b=2, coeffs=co.data_ptr(), times=ti.data_ptr(), sb=3, sk=1, cons=ctypes.byref(c), out=traj.data_ptr(), bounds=None):
        return ctx.lib.mtg_check_input_feasibility_recursive(ctx.handle, n, k, d, b, coeffs, times, sb, sk, cons, out, None, None, bounds, None)

    for bad in (dict(n=4), dict(n=13), dict(k=0), dict(d=0), dict(b=-1), dict(coeffs=None), dict(times=None), dict(cons=None),
                dict(out=None), dict(sb=0), dict(sk=-1), dict(sb=2, sk=1), dict(bounds=8)):
        assert call(**bad) == -1, bad
    assert call(n=13) == -1 and b"n_coeffs must be in [5,12]" in ctx.lib.mtg_last_error_string(ctx.handle)
    assert call(bounds=8) == -1 and b"16-byte aligned" in ctx.lib.mtg_last_error_string(ctx.handle)
    assert call(b=0) == 0                                           # a B = 0 call: fine, and nothing runs
    ctx.sync()
    assert (traj.cpu().numpy() == -7).all()
    assert call() == 0
    ctx.sync()
    assert (traj.cpu().numpy() == 0).all()                          # hover: feasible under the default limits
    # dimension 2: indeterminable everywhere
    out = m.check_input_feasibility_recursive(ctx, torch.zeros((5, 3, 2, 10), dtype=torch.float64, device="cuda"),
                                              torch.ones((5, 3), dtype=torch.float64, device="cuda"), m.InputConstraints.defaults(),
                                              want_sections=True)
    ctx.sync()
    assert (out[0].cpu().numpy() == 1).all() and (out[1].cpu().numpy() == 0).all() and (out[2].cpu().numpy() == 1).all()
    assert np.isnan(out[3].cpu().numpy()).all() and (out[4].cpu().numpy() == 0).all()
