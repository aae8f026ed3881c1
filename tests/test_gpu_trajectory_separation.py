"""Trajectory-to-trajectory separation check on the device (mtg_check_trajectory_separation, csrc/mtg_separation.hip): against the
library's host build of the same lane code at the smallest shapes where the kernel could go wrong -- every instantiation at
one full workgroup plus one lane, one segment on side A, the two sides in the same buffers, [K][B] times, null starts, null
optional outputs, a pair index out of range -- its argument table, and captured into a graph."""
import numpy as np
import pytest

import trajectory_separation_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import mav_trajectory_generation_amd as m
    c = m.Context(0)
    yield c
    c.close()


def on_device(ctx, z, layout="aos", same_buffers=False, **kw):
    import torch
    import mav_trajectory_generation_amd as m
    dev = lambda a: None if a is None else torch.from_numpy(np.array(a)).cuda()
    lay = lambda t: t if layout == "aos" else np.ascontiguousarray(t.T)
    args = dict(kw)
    start_a, start_b = args.pop("start_a", z["start_a"]), args.pop("start_b", z["start_b"])
    ca, ta, sa = dev(z["coeffs_a"]), dev(lay(z["times_a"])), dev(start_a)
    cb, tb, sb = (ca, ta, sa) if same_buffers else (dev(z["coeffs_b"]), dev(lay(z["times_b"])), dev(start_b))
    out = m.check_trajectory_separation(ctx, ca, ta, cb, tb, dev(z["pairs"]), z["min_separation"], start_a=sa, start_b=sb, times_layout=layout,
                                        **args)
    ctx.sync()
    return m.TrajectorySeparationResult(*[o.cpu().numpy() if o is not None else None for o in out])


def same_as_host(ctx, z, layout="aos", same_buffers=False, **kw):
    """Device against host form: verdicts, every index column and the piece counts equal, values within 1e-9 max(1, scale); returns
    the device result."""
    import mav_trajectory_generation_amd as m
    args = dict(start_a=z["start_a"], start_b=z["start_b"])
    args.update(kw)
    h = m.check_trajectory_separation_host(z["coeffs_a"], z["times_a"], z["coeffs_b"], z["times_b"], z["pairs"], z["min_separation"], **args)
    d = on_device(ctx, z, layout, same_buffers, **kw)
    for name in ("pair_feasible", "first_failing_segment_a", "first_failing_segment_b", "pair_closest_segment_a", "pair_closest_segment_b",
                 "segment_closest_segment_b", "segment_pieces"):
        assert np.array_equal(getattr(d, name), getattr(h, name)), name
    scale = R.scale_of(z["coeffs_a"], z["times_a"], z["coeffs_b"], z["times_b"], z["pairs"], z["min_separation"])
    bound = 1e-9 * np.maximum(1.0, np.where(np.isfinite(scale), scale, 1.0))      # (a pair with a NaN input has no finite value to bound)
    worst = 0.0
    for name in ("pair_separation", "pair_closest_time", "segment_separation", "segment_closest_time"):
        x, y = getattr(d, name), getattr(h, name)
        b = bound if x.ndim == 1 else bound[:, None]
        assert np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(np.isinf(x), np.isinf(y)), name
        fin = np.isfinite(y)
        err = np.abs(np.where(fin, x, 0.0) - np.where(fin, y, 0.0))
        worst = max(worst, float((err / b).max()))
        assert (err <= b).all(), (name, float(err.max()))
    print(f"device vs host: largest share of the bound {worst:.2e}")
    return d


@pytest.mark.parametrize("n", [3, 4, 5, 6, 7, 8, 10, 12])
@pytest.mark.parametrize("family", R.FAMILIES)
def test_every_instantiation_at_65_lanes(ctx, n, family):
    """13 pairs x 5 segments of A: one full workgroup plus one lane, in the instantiations 4, 6, 8, 10, 12 (odd and small N
    zero-padded); Kb = 4, 3 and 7."""
    d = 4 if n in (5, 8, 12) else 3
    r = same_as_host(ctx, R.reference(n, d, family))
    if family == "far":
        assert r.pair_feasible.all()
    if family == "crossing":
        assert not r.pair_feasible.all()


@pytest.mark.parametrize("name", ["n10_k8_d3_fast", "n10_k2_d3", "n12_k4_d4", "n7_k4_d4"])
def test_device_entry_vs_reference(ctx, name):
    """The reference's own candidates and evaluation on 60 pairs of its own trajectories, both sides the same tensors: N = 10, 12
    and the zero-padded 7, K = 8, 2, 4, D = 3 and 4."""
    import torch
    import mav_trajectory_generation_amd as m
    from test_trajectory_separation_golden import check_against_fixture

    def run(coeffs, times, start, pairs, msep):
        co, ti, st = (torch.from_numpy(np.array(a)).cuda() for a in (coeffs, times, start))
        out = m.check_trajectory_separation(ctx, co, ti, co, ti, torch.from_numpy(np.array(pairs)).cuda(), msep, start_a=st, start_b=st)
        ctx.sync()
        return m.TrajectorySeparationResult(*[o.cpu().numpy() for o in out])
    check_against_fixture(name, run)


def test_one_segment_on_side_a(ctx):
    z = R.make_inputs(10, 3, "random", ka=1, kb=9)
    r = same_as_host(ctx, z)
    assert r.segment_separation.shape == (R.P, 1) and r.segment_pieces.max() > 1
    same_as_host(ctx, R.make_inputs(7, 3, "random", ka=9, kb=1))


def test_same_buffers_and_distinct_buffers(ctx):
    """A swarm against itself: both sides are the same tensors; and the same numbers in two allocations."""
    z = R.make_inputs(10, 3, "random", ka=5, kb=5, ba=7, bb=7)
    z.update(coeffs_b=z["coeffs_a"], times_b=z["times_a"], start_b=z["start_a"])
    z["pairs"] = np.concatenate([z["pairs"][:10], [[2, 2], [0, 6], [6, 0]]]).astype(np.int32)
    same = same_as_host(ctx, z, same_buffers=True)
    distinct = same_as_host(ctx, z)
    for x, y in zip(same, distinct):
        assert np.array_equal(x, y, equal_nan=True)
    assert same.pair_separation[10] == -z["min_separation"] and same.pair_feasible[10] == 0


def test_soa_times_null_starts_and_absent_outputs(ctx):
    import torch
    z = R.reference(8, 3, "random")
    aos = same_as_host(ctx, z)
    soa = same_as_host(ctx, z, layout="soa")
    for x, y in zip(aos, soa):
        assert np.array_equal(x, y, equal_nan=True)
    same_as_host(ctx, z, start_a=None, start_b=None)
    same_as_host(ctx, z, start_a=None)
    few = on_device(ctx, z, want_closest=False)
    assert all(x is None for x in few[4:])
    for x, y in zip(few[:4], aos[:4]):
        assert np.array_equal(x, y, equal_nan=True)
    # all optional outputs null but the required one
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    ca, ta, sa, cb, tb, sb, pairs = (dev(z[k]) for k in ("coeffs_a", "times_a", "start_a", "coeffs_b", "times_b", "start_b", "pairs"))
    feas = torch.full((R.P,), -7, dtype=torch.int32, device="cuda")
    ka, kb = z["coeffs_a"].shape[1], z["coeffs_b"].shape[1]
    assert ctx.lib.mtg_check_trajectory_separation(ctx.handle, 8, 3, ka, R.BA, ca.data_ptr(), ta.data_ptr(), ka, 1, sa.data_ptr(), kb, R.BB,
                                                   cb.data_ptr(), tb.data_ptr(), kb, 1, sb.data_ptr(), R.P, pairs.data_ptr(),
                                                   z["min_separation"], feas.data_ptr(), *([None] * 10)) == 0
    ctx.sync()
    assert np.array_equal(feas.cpu().numpy(), aos.pair_feasible)


def test_degenerate_pairs(ctx):
    """An empty window, a window that touches at an instant, unusable times: the rules of the host form, on the device."""
    z = R.make_inputs(10, 3, "random")
    a0, b0 = (int(x) for x in z["pairs"][0])
    z["start_b"][b0] = R.breakpoints(z["times_a"][a0], z["start_a"][a0])[-1]        # pair 0 touches at an instant: no piece
    z["start_b"][(b0 + 5) % R.BB] = 1000.0                                          # never at the same time as anybody
    z["times_a"][(a0 + 1) % R.BA, 2] = -0.25
    z["times_a"][(a0 + 2) % R.BA, 0] = np.nan
    z["coeffs_a"][(a0 + 4) % R.BA, 1, 0, 0] = np.nan
    r = same_as_host(ctx, z)
    assert r.pair_feasible[0] == 1 and r.pair_separation[0] == np.inf and (r.segment_pieces[0] == 0).all()
    invalid = np.isin(z["pairs"][:, 0], [(a0 + 1) % R.BA, (a0 + 2) % R.BA])
    assert np.isnan(r.pair_separation[invalid]).all() and not r.pair_feasible[invalid].any() and (r.segment_pieces[invalid] == 0).all()
    empty = (z["pairs"][:, 1] == (b0 + 5) % R.BB) & ~invalid
    assert empty.any() and invalid.any() and np.isnan(r.pair_separation).sum() > invalid.sum()
    assert (r.pair_separation[empty] == np.inf).all() and r.pair_feasible[empty].all()


def test_pair_index_guard(ctx):
    """Side A is allocated for 8 trajectories and passed as a batch of 4; a pair that names index 5 reads nothing and comes back NaN
    and infeasible.  The memory is valid either way: a missing guard shows as a wrong answer."""
    import torch
    z = R.make_inputs(10, 3, "random", ka=5, kb=4, ba=8, bb=6)
    pairs = z["pairs"].copy()
    pairs[:, 0] %= 4
    pairs[3], pairs[7], pairs[9], pairs[12] = (5, 1), (4, 0), (1, 6), (-1, 2)
    bad = np.zeros(R.P, dtype=bool)
    bad[[3, 7, 9, 12]] = True
    import mav_trajectory_generation_amd as m
    h = m.check_trajectory_separation_host(z["coeffs_a"][:4], z["times_a"][:4], z["coeffs_b"], z["times_b"], pairs[~bad], z["min_separation"],
                                           start_a=z["start_a"][:4], start_b=z["start_b"])
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    ca, ta, sa, cb, tb, sb, pr = (dev(a) for a in (z["coeffs_a"], z["times_a"], z["start_a"], z["coeffs_b"], z["times_b"], z["start_b"], pairs))
    d = m.check_trajectory_separation(ctx, ca[:4], ta[:4], cb, tb, pr, z["min_separation"], start_a=sa[:4], start_b=sb)
    ctx.sync()
    d = m.TrajectorySeparationResult(*[o.cpu().numpy() for o in d])
    assert not d.pair_feasible[bad].any() and np.isnan(d.pair_separation[bad]).all() and np.isnan(d.pair_closest_time[bad]).all()
    assert np.isnan(d.segment_separation[bad]).all() and (d.segment_pieces[bad] == 0).all() and (d.segment_closest_segment_b[bad] == -1).all()
    for out in (d.first_failing_segment_a, d.first_failing_segment_b, d.pair_closest_segment_a, d.pair_closest_segment_b):
        assert (out[bad] == -1).all()
    bound = 1e-9 * np.maximum(1.0, R.scale_of(z["coeffs_a"], z["times_a"], z["coeffs_b"], z["times_b"], pairs[~bad], z["min_separation"]))
    assert np.array_equal(d.pair_feasible[~bad], h.pair_feasible) and np.array_equal(d.segment_pieces[~bad], h.segment_pieces)
    assert (np.abs(d.pair_separation[~bad] - h.pair_separation) <= bound).all()


def test_argument_errors_enqueue_nothing(ctx):
    import torch
    z = R.reference(10, 3, "random")
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    ca, ta, sa, cb, tb, sb, pairs = (dev(z[k]) for k in ("coeffs_a", "times_a", "start_a", "coeffs_b", "times_b", "start_b", "pairs"))
    ka, kb = z["coeffs_a"].shape[1], z["coeffs_b"].shape[1]
    feas = torch.full((R.P,), -7, dtype=torch.int32, device="cuda")
    time = torch.zeros((R.P,), dtype=torch.float64, device="cuda")

    def call(n=10, d=3, ka=ka, ba=R.BA, tsa=(ka, 1), kb=kb, bb=R.BB, tsb=(kb, 1), n_pairs=R.P, msep=1.0, coeffs_a=ca.data_ptr(),
             pairs_ptr=pairs.data_ptr(), feasible=feas.data_ptr(), closest_time=None):
        return ctx.lib.mtg_check_trajectory_separation(ctx.handle, n, d, ka, ba, coeffs_a, ta.data_ptr(), *tsa, sa.data_ptr(), kb, bb,
                                                       cb.data_ptr(), tb.data_ptr(), *tsb, sb.data_ptr(), n_pairs, pairs_ptr, msep, feasible,
                                                       None, None, None, closest_time, *([None] * 6))
    for bad in (dict(n=0), dict(n=13), dict(d=2), dict(d=5), dict(ka=0), dict(ka=1025), dict(kb=0), dict(kb=1025), dict(ba=-1), dict(bb=-1),
                dict(tsa=(0, 1)), dict(tsa=(ka, 0)), dict(tsa=(ka - 1, 1)), dict(tsb=(kb, -1)), dict(tsb=(1, R.BB - 1)), dict(n_pairs=-1),
                dict(n_pairs=(1 << 31) // ka + 1), dict(msep=-1.0), dict(msep=float("nan")), dict(msep=float("inf")), dict(coeffs_a=None),
                dict(pairs_ptr=None), dict(feasible=None), dict(closest_time=time.data_ptr())):
        assert call(**bad) == -1, bad
    assert b"trajectory separation" in ctx.lib.mtg_last_error_string(ctx.handle)
    assert call(n_pairs=0) == 0
    ctx.sync()
    assert (feas.cpu().numpy() == -7).all()


def test_capture_and_replay(ctx):
    """The call is three kernel launches on the context's stream: captured once, replayed once on new coefficients."""
    import torch
    import mav_trajectory_generation_amd as m
    z = R.reference(10, 3, "random")
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    ca, ta, sa, cb, tb, sb, pairs = (dev(z[k]) for k in ("coeffs_a", "times_a", "start_a", "coeffs_b", "times_b", "start_b", "pairs"))
    ka, kb = z["coeffs_a"].shape[1], z["coeffs_b"].shape[1]
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    out = [i32(R.P), i32(R.P), i32(R.P), f64(R.P), f64(R.P), i32(R.P), i32(R.P), f64(R.P, ka), f64(R.P, ka), i32(R.P, ka), i32(R.P, ka)]

    def call():
        assert ctx.lib.mtg_check_trajectory_separation(ctx.handle, 10, 3, ka, R.BA, ca.data_ptr(), ta.data_ptr(), ka, 1, sa.data_ptr(), kb, R.BB,
                                                       cb.data_ptr(), tb.data_ptr(), kb, 1, sb.data_ptr(), R.P, pairs.data_ptr(),
                                                       z["min_separation"], *[o.data_ptr() for o in out]) == 0
    torch.cuda.synchronize()
    call()                                       # warm-up outside the capture (module load)
    ctx.sync()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(ctx.stream):
        with torch.cuda.graph(g, stream=ctx.stream):
            call()
    ca.copy_(torch.flip(ca, dims=(0,)))          # new values in the captured buffers
    ta.copy_(torch.flip(ta, dims=(0,)))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    replayed = [o.cpu().numpy().copy() for o in out]
    call()                                       # the eager call on the same new values
    ctx.sync()
    for x, y in zip(replayed, out):
        assert np.array_equal(x, y.cpu().numpy(), equal_nan=True)
    h = m.check_trajectory_separation_host(z["coeffs_a"][::-1], z["times_a"][::-1], z["coeffs_b"], z["times_b"], z["pairs"], z["min_separation"],
                                           start_a=z["start_a"], start_b=z["start_b"])
    assert np.array_equal(replayed[0], h.pair_feasible) and np.array_equal(replayed[10], h.segment_pieces)
