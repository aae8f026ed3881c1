"""mtg_sample_range (csrc/mtg_sample.hip) against the longdouble reference tests/sampling_ref.py: every compile-time-shape
kernel in the steady state of its software pipeline, the run-time-shape kernel through several grid-stride steps, samples exactly
on vertices / on the end time / before 0, the rounding of the sample times, the shipped grid over several sweeps, and the
argument checks of the C entry.

Inputs: coefficients are RANDOM (standard normal x 10^uniform(-3, 3), independent per segment), not solved trajectories:
neighbouring segments are discontinuous, so a sample that reads the wrong segment's or the wrong lane's coefficients is off by
O(1) instead of by rounding.  Segment times lie in [0.3, 3] unless a test says otherwise.

Acceptance, every value:  |got - want| <= (2N + ND + 2) * 2^-53 * p~_m,  p~_m = m! sum_j C(j, m) |c_j| |local|^(j-m).
Derivation: the kernels run  a[m] <- a[m] * t + a[m-1]  (m = ND-1 .. 1),  a[0] <- a[0] * t + c_j  for j = N-1 .. 0.  The
contribution of c_j to the final a[m] enters at step j and passes through exactly one multiply-add in each of the <= N steps
it lives through, being multiplied by t (it stays in its a[k]) or added (it moves up to a[k+1], which happens m times): at
most N multiplies and N + m <= N + ND adds, each rounded once when not fused (fused, a multiply-add rounds once: fewer).  Then
come the multiplication with m! and the final rounding of the stored value: (2N + ND + 2) roundings, each a relative
perturbation <= u = 2^-53 of a term whose magnitudes sum to p~_m.  (First order in u; the neglected (n u)^2 / 2 part is 1e-29
of p~.)  The reference itself is within (2N + 2) 2^-64 p~_m (tests/test_sampling_ref.py).  No value is left out.

Every launch writes into NaN-filled buffers followed by 64 guard words (out and n_valid alike), must leave no NaN and no
touched guard, and is run with both time layouts, which must agree bit for bit."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import sampling_ref as sr

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GUARD = 64
VALID_FILL = -(2 ** 31)


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import mav_trajectory_generation_amd as m
    c = m.Context(0)
    yield c
    c.close()


def random_case(rng, bsz, k, dim, n):
    coeffs = rng.standard_normal((bsz, k, dim, n)) * 10.0 ** rng.uniform(-3, 3, (bsz, k, dim, n))
    times = rng.uniform(0.3, 3.0, (bsz, k))
    return coeffs, times


def grid_for(times, S):
    """(t_start, dt): starts before 0, and the average trajectory ends at about 80 % of the grid (the short ones run far past
    their end, the long ones never reach it)."""
    if S == 1:
        return 0.83, 0.61
    return -0.37, float(times.sum(axis=1).mean()) / (0.8 * S)


def launch(ctx, co, t, t_start, dt, S, nd):
    """One guarded launch per time layout -> (out [B][S][ND][D], n_valid [B]) device tensors (of the AoS launch)."""
    import torch
    import mav_trajectory_generation_amd as m
    bsz, _, dim, _ = co.shape
    numel = bsz * S * nd * dim
    res = []
    for layout, tt in (("aos", t), ("soa", t.t().contiguous())):
        buf = torch.full((numel + GUARD,), float("nan"), dtype=torch.float64, device=co.device)
        vbuf = torch.full((bsz + GUARD,), VALID_FILL, dtype=torch.int32, device=co.device)
        out, nv = m.sample_range(ctx, co, tt, t_start, dt, S, nd, times_layout=layout, out=buf[:numel], valid=vbuf[:bsz])
        ctx.sync()
        assert out.data_ptr() == buf.data_ptr() and nv.data_ptr() == vbuf.data_ptr()
        assert not bool(torch.isnan(out).any()), "a row of `out` was not written"
        assert bool(torch.isnan(buf[numel:]).all()), "write past the end of `out`"
        assert bool((nv != VALID_FILL).all()), "an element of `n_valid` was not written"
        assert bool((vbuf[bsz:] == VALID_FILL).all()), "write past the end of `n_valid`"
        res.append((out, nv))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), "AoS and SoA time layouts differ"
    return res[0]


def assert_within_bound(got, want, scale, n, nd, what):
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    bound = (2 * n + nd + 2) * U * scale
    bad = err > bound
    print("%s: max err / bound = %.3g over %d values" % (what, float((err / np.where(bound > 0, bound, 1.0)).max()), err.size))
    n_bad = int(bad.sum())
    assert n_bad == 0, "%s: %d values outside the bound, first at %s, worst err / bound = %.3g" % (
        what, n_bad, np.argwhere(bad)[:5].tolist(), float((err[bad] / np.maximum(bound[bad], 1e-300)).max()))


def check(ctx, coeffs, times, t_start, dt, S, nd, what):
    """Guarded launch of both layouts, whole output and n_valid against the reference -> (out, n_valid) device tensors."""
    import torch
    out, nv = launch(ctx, torch.from_numpy(coeffs).cuda(), torch.from_numpy(times).cuda(), t_start, dt, S, nd)
    want, scale, want_nv, _, _ = sr.sample_ref(coeffs, times, t_start, dt, S, nd)
    assert_within_bound(out.cpu().numpy(), want, scale, coeffs.shape[3], nd, what)
    assert np.array_equal(nv.cpu().numpy(), want_nv), what
    return out, nv


class knobs:
    """Measurement knobs of the context for one block; restored to the shipped values whatever happens."""

    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, kw

    def __enter__(self):
        try:
            for name, value in self.kw.items():
                self.ctx.set_option(name, value)
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        for name in self.kw:
            self.ctx.set_option(name, 0)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim", [(10, 3), (12, 3), (8, 3), (10, 1), (10, 4), (12, 4)])
def test_every_ct_kernel_in_pipeline_steady_state(ctx, n, dim):
    """All 10 instantiations mtg_sample_kernel_ct<ND, N, D, KMAX> of one (N, D) (ND = 1..5; K = 5 -> KMAX 8, K = 13 -> KMAX 16)
    with the grid capped at 2 workgroups = 8 wave-workers: B x S = 39 x 45 = 1755 = 64 * 27 + 27 samples are 27 full chunks --
    workers 0..2 run four pipeline steps, 3..7 three, all of them request chunks past the end -- plus a partial chunk owned by
    worker 27 % 8 = 3, which has done pipeline work before.  (S = 45 admits no B with a 37-sample tail; 27 full chunks and the
    owner of the tail are what matters.)  Then the run-time-shape kernel on the same inputs: the same sequence of fused
    multiply-adds, so the two must agree bit for bit.
    (Even ND * D is a compile-time kernel like any other -- <2, 10, 3, 8> is one; the shape comment in
    tests/test_gpu_parity.py::test_batched_sampling_vs_oracle that sends it to the run-time-shape kernel is out of date.)"""
    import torch
    rng = np.random.default_rng(1000 * n + dim)
    bsz, S = 39, 45
    assert bsz * S == 64 * 27 + 27
    for k in (5, 13):
        coeffs, times = random_case(rng, bsz, k, dim, n)
        t_start, dt = grid_for(times, S)
        for nd in range(1, 6):
            what = "ct N=%d D=%d K=%d ND=%d" % (n, dim, k, nd)
            with knobs(ctx, sample_max_blocks=2):
                out_ct, nv_ct = check(ctx, coeffs, times, t_start, dt, S, nd, what)
            with knobs(ctx, sample_max_blocks=2, sample_generic=1):
                out_rt, nv_rt = check(ctx, coeffs, times, t_start, dt, S, nd, what + " (run-time-shape kernel)")
            assert torch.equal(out_ct, out_rt) and torch.equal(nv_ct, nv_rt), what


@pytest.mark.parametrize("n,dim,k,nd,S,bsz,generic", [
    (2, 2, 1, 5, 1, 1601, 0),       # S = 1: a chunk spans 64 trajectories; ND > N: derivatives 2.. are exactly 0
    (6, 5, 17, 3, 7, 231, 0),       # a chunk spans 10 trajectories, blk_s wraps in most steps
    (11, 2, 40, 4, 64, 26, 0),      # a chunk is exactly one trajectory; total a multiple of 64
    (11, 5, 17, 2, 200, 9, 0),      # chunks inside one trajectory
    (6, 1, 17, 1, 7, 240, 0),       # R = 1: half the lanes of the write-out store nothing
    (10, 1, 5, 1, 7, 240, 1),       # R = 1 on a shape that has a compile-time kernel, forced to the run-time one
    (6, 12, 17, 5, 200, 8, 0),      # R = 60
    (2, 12, 40, 5, 64, 26, 0),      # R = 60, N = 2
    (11, 5, 1, 5, 7, 233, 0),       # R = 25, one segment
])
def test_runtime_shape_kernel_grid_stride(ctx, n, dim, k, nd, S, bsz, generic):
    """mtg_sample_kernel<ND> with 8 wave-workers: 512 samples per step, every launch >= 1537 samples, i.e. >= 3 full steps of
    the grid-stride loop plus a partial one -- the incremental (blk_b, blk_s) advance with and without wrap, the prefetch of the
    next chunk's site before the stores of this one, LDS slab reuse, lanes past the end of the launch."""
    assert bsz * S > 3 * 8 * 64
    rng = np.random.default_rng(7919 * n + 31 * dim + k + S)
    coeffs, times = random_case(rng, bsz, k, dim, n)
    t_start, dt = grid_for(times, S)
    with knobs(ctx, sample_max_blocks=2, sample_generic=generic):
        check(ctx, coeffs, times, t_start, dt, S, nd, "rt N=%d D=%d K=%d ND=%d S=%d" % (n, dim, k, nd, S))


def exact_grid_times(rng, bsz, k, total_units):
    """Segment times in multiples of 1/8; the first half of the trajectories all last total_units / 8."""
    units = rng.integers(2, 7, (bsz, k))
    units[: bsz // 2, -1] = total_units - units[: bsz // 2, :-1].sum(axis=1)
    assert units.min() >= 2
    return units * 0.125, units


@pytest.mark.parametrize("n,dim,k,nd,generic", [(10, 3, 8, 5, 0), (10, 3, 8, 5, 1), (6, 2, 5, 3, 0)])
def test_exact_grid_vertices_end_and_before_start(ctx, n, dim, k, nd, generic):
    """Segment times in multiples of 0.125, dt in {0.125, 0.25}, t_start in {0, 0.375, -0.5, total, total + 1}: every t_i and
    every prefix sum is exact in any rounding, so the expectations are unambiguous:
      * a sample on an interior vertex is the RIGHT-hand segment at local time 0: exactly m! c_m of that segment;
      * the sample at the end time is the last segment at its end, later samples equal it bit for bit;
      * t_i < 0 extrapolates segment 0 (negative local time): the present behaviour, pinned here;
      * n_valid is the reference count: 0 for t_start past the end, 1 for t_start == total, and with S = 1."""
    total_units = 48                                  # 6.0
    rng = np.random.default_rng(99 + n + k)
    bsz = 40
    coeffs = rng.standard_normal((bsz, k, dim, n)) * 10.0 ** rng.uniform(-3, 3, (bsz, k, dim, n))
    times, units = exact_grid_times(rng, bsz, k, total_units)
    ends = np.cumsum(units, axis=1)
    total = total_units * 0.125
    assert (np.cumsum(times, axis=1)[: bsz // 2, -1] == total).all()
    fact = np.array([1.0, 1.0, 2.0, 6.0, 24.0])[:nd]
    seen = dict(vertex=0, end=0, past=0, negative=0)
    with knobs(ctx, sample_max_blocks=2, sample_generic=generic):
        for dt_units, S in ((1, 70), (2, 40), (1, 1)):
            for t0 in (0.0, 0.375, -0.5, total, total + 1.0):
                dt = dt_units * 0.125
                what = "exact grid N=%d K=%d dt=%g t_start=%g S=%d" % (n, k, dt, t0, S)
                out, nv = check(ctx, coeffs, times, t0, dt, S, nd, what)
                got, nv = out.cpu().numpy(), nv.cpu().numpy()
                _, _, _, seg, local = sr.sample_ref(coeffs, times, t0, dt, S, nd)
                tu = int(round(t0 * 8)) + dt_units * np.arange(S)                       # sample times in units of 1/8
                for b in range(bsz):
                    for s in range(S):
                        if tu[s] in ends[b, :-1]:                                       # interior vertex
                            kk = int(np.searchsorted(ends[b], tu[s])) + 1
                            assert seg[b, s] == kk and local[b, s] == 0.0
                            assert np.array_equal(got[b, s], (coeffs[b, kk, :, :nd] * fact).T), (what, b, s)
                            seen["vertex"] += 1
                        elif tu[s] >= ends[b, -1]:                                      # end time and beyond
                            assert seg[b, s] == k - 1 and local[b, s] == times[b, -1]
                            first = int(np.argmax(tu >= ends[b, -1]))
                            assert np.array_equal(got[b, s], got[b, first]), (what, b, s)
                            seen["end" if tu[s] == ends[b, -1] else "past"] += 1
                        elif tu[s] < 0:
                            assert seg[b, s] == 0 and local[b, s] == tu[s] * 0.125
                            seen["negative"] += 1
                    assert nv[b] == int((tu <= ends[b, -1]).sum())
                if t0 == total:
                    assert (nv[: bsz // 2] == 1).all()
                if t0 == total + 1.0:
                    assert (nv[: bsz // 2] == 0).all()
    assert min(seen.values()) > 100, seen


def find_rounding_triples():
    """(t_start, dt, i, two-rounding t_i) whose single-rounding (fused) t_i lies one ulp BELOW / ABOVE fl(t_start + fl(i dt))."""
    below = above = None
    for t0 in (0.1, 0.3, 0.7, 1.3):
        for dt in (0.1, 0.01, 0.37, 0.05):
            for i in range(1, 200):
                two = t0 + dt * i
                fused = float(Fraction(t0) + Fraction(dt) * i)          # exact, then rounded once
                if two < 1.0:
                    continue                                            # (the constructions below want room for segments)
                if below is None and fused == np.nextafter(two, -np.inf):
                    below = (t0, dt, i, two)
                if above is None and fused == np.nextafter(two, np.inf):
                    above = (t0, dt, i, two)
    return below, above


@pytest.mark.parametrize("generic", [0, 1])
def test_sample_time_is_rounded_twice(ctx, generic):
    """t_i = fl(t_start + fl(i dt)) (include/mtg_hip.h), not the fused value.  Triples where the two differ by one ulp are
    searched for, not hard-coded.  (a) fused one ulp BELOW: with the first segment time set to the two-rounding t_i, `acc > t`
    is false at segment 0, so sample i is segment 1 at local time 0 -- a fused t would evaluate segment 0 at its end, an O(1)
    different value.  (b) fused one ulp ABOVE: with the total time equal to the two-rounding t_i, sample i counts in n_valid.
    Segment times here are what the constructions need, not [0.3, 3]."""
    below, above = find_rounding_triples()
    assert below is not None and above is not None
    n, dim, nd, bsz = 10, 3, 5, 8
    rng = np.random.default_rng(5)
    fact = np.array([1.0, 1.0, 2.0, 6.0, 24.0])
    with knobs(ctx, sample_generic=generic):
        # (a)
        t0, dt, i, two = below
        S = max(i + 2, 16)
        coeffs, times = random_case(rng, bsz, 5, dim, n)
        times[:, 0] = two
        out, _ = check(ctx, coeffs, times, t0, dt, S, nd, "t_i below, generic=%d" % generic)
        _, _, _, seg, local = sr.sample_ref(coeffs, times, t0, dt, S, nd)
        assert (seg[:, i] == 1).all() and (local[:, i] == 0.0).all()
        assert np.array_equal(out.cpu().numpy()[:, i], np.swapaxes(coeffs[:, 1, :, :nd] * fact, 1, 2))
        # (b): three segments, the first two exact multiples of 1/8 that sum to at least half of t_i (then the last one,
        # t_i minus their sum, is exact and the float64 prefix sum ends on t_i exactly)
        t0, dt, i, two = above
        S = max(i + 2, 16)
        coeffs, times = random_case(rng, bsz, 3, dim, n)
        q = np.round(two / 3.0 * 8.0) * 0.125
        times[:, 0], times[:, 1] = q, q
        times[:, 2] = two - 2 * q
        assert (times > 0).all() and (np.cumsum(times, axis=1)[:, -1] == two).all()
        _, nv = check(ctx, coeffs, times, t0, dt, S, nd, "t_i above, generic=%d" % generic)
        assert (nv.cpu().numpy() == i + 1).all()


@pytest.mark.parametrize("n,dim,k,nd", [(10, 3, 8, 5), (6, 3, 8, 3)])
def test_shipped_grid_several_sweeps(ctx, n, dim, k, nd):
    """No cap: the grid the library ships (occupancy x CUs workgroups).  One sweep is at most CUs x 8 workgroups (the most a CU
    holds at 256 threads) x 4 waves x 64 samples; 2.3 sweeps + 37 samples run every wave through >= 2 steps.  The whole output
    must equal, bit for bit, the same launch on 64 workgroups (each wave then runs ~75 steps); the first and last 256 samples
    and 20 000 random ones are checked against the reference."""
    import torch
    S = 97
    sweep = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 4 * 64
    bsz = int(round((2.3 * sweep + 37) / S))
    total = bsz * S
    rng = np.random.default_rng(2024 + n)
    coeffs, times = random_case(rng, bsz, k, dim, n)
    t_start, dt = grid_for(times, S)
    co, t = torch.from_numpy(coeffs).cuda(), torch.from_numpy(times).cuda()
    out, nv = launch(ctx, co, t, t_start, dt, S, nd)
    with knobs(ctx, sample_max_blocks=64):
        out64, nv64 = launch(ctx, co, t, t_start, dt, S, nd)
    assert torch.equal(out, out64) and torch.equal(nv, nv64)
    del out64
    idx = np.unique(np.concatenate([np.arange(256), np.arange(total - 256, total), rng.integers(0, total, 20000)]))
    b_idx, s_idx = idx // S, idx % S
    want, scale, want_nv, _, _ = sr.sample_ref(coeffs, times, t_start, dt, S, nd, pairs=(b_idx, s_idx))
    got = out.view(total, nd, dim)[torch.from_numpy(idx).cuda()].cpu().numpy()
    assert_within_bound(got, want, scale, n, nd, "shipped grid N=%d D=%d: %d samples" % (n, dim, total))
    assert np.array_equal(nv.cpu().numpy(), want_nv)


def test_argument_table_of_the_c_entry(ctx):
    """mtg_sample_range returns before any launch on every rejected call (the NaN-filled buffers stay NaN), batch = 0 is
    MTG_OK with nothing written, and the "sample_max_blocks" knob is set like every other knob."""
    import torch
    import mav_trajectory_generation_amd as m
    INVALID, UNSUPPORTED = -1, -6
    bsz, k, S = 4, 3, 8
    co = torch.ones((bsz * k * 16 * 13,), dtype=torch.float64, device="cuda")
    t = torch.ones((bsz * k,), dtype=torch.float64, device="cuda")
    out = torch.full((bsz * S * 65 + 2,), float("nan"), dtype=torch.float64, device="cuda")
    nv = torch.full((bsz,), VALID_FILL, dtype=torch.int32, device="cuda")
    assert out.data_ptr() % 16 == 0

    def call(n=10, dim=3, batch=bsz, dt=0.5, nd=5, offset=0):
        return ctx.lib.mtg_sample_range(ctx.handle, n, k, dim, batch, ctypes.c_void_p(co.data_ptr()), ctypes.c_void_p(t.data_ptr()),
                                        k, 1, 0.0, dt, S, nd, ctypes.c_void_p(out.data_ptr() + offset), ctypes.c_void_p(nv.data_ptr()))

    for dt in (0.0, -1.0, float("nan")):
        assert call(dt=dt) == INVALID
    for n in (1, 13):
        assert call(n=n) == INVALID
    assert call(offset=8) == INVALID
    assert call(nd=6) == UNSUPPORTED
    assert call(nd=5, dim=13) == UNSUPPORTED               # ND * D = 65
    assert call(batch=0) == 0
    ctx.sync()
    assert bool(torch.isnan(out).all()) and bool((nv == VALID_FILL).all())
    assert call(offset=16) == 0                            # the same call, valid: it does write
    ctx.sync()
    assert not bool(torch.isnan(out[2:2 + bsz * S * 15]).any()) and bool(torch.isnan(out[:2]).all())
    assert bool(torch.isnan(out[2 + bsz * S * 15:]).all()) and bool((nv == 7).all())   # t_i <= 3.0: i = 0..6
    # the knob: a valid value, clamped below at 0 (= shipped), an unknown name
    lib = ctx.lib
    try:
        assert lib.mtg_context_set_option(ctx.handle, b"sample_max_blocks", 3) == 0
        assert lib.mtg_context_set_option(ctx.handle, b"sample_max_blocks", -5) == 0
        assert lib.mtg_context_set_option(ctx.handle, b"sample_max_block", 1) == INVALID
        assert b"unknown option" in lib.mtg_last_error_string(ctx.handle)
        assert lib.mtg_context_set_option(None, b"sample_max_blocks", 1) == INVALID
        with pytest.raises(m.MtgError):
            ctx.set_option("sample_max_block", 1)
    finally:
        ctx.set_option("sample_max_blocks", 0)
    # caller-supplied buffers of the Python layer
    co4 = co[: bsz * k * 3 * 10].view(bsz, k, 3, 10)
    t2 = t.view(bsz, k)
    good = torch.empty((bsz * S * 15 + 2,), dtype=torch.float64, device="cuda")
    numel = bsz * S * 15
    for bad_out in (good[: numel - 1],                                                   # size
                    good[1: numel + 1],                                                  # 8 bytes off a 16-byte boundary
                    good[:numel].float(), good[:numel].cpu(),                            # dtype, device
                    torch.empty((2 * numel,), dtype=torch.float64, device="cuda")[::2]):  # not contiguous
        with pytest.raises(ValueError):
            m.sample_range(ctx, co4, t2, 0.0, 0.5, S, 5, out=bad_out)
    for bad_valid in (nv[:-1], nv.long(), nv.cpu(), torch.empty((2 * bsz,), dtype=torch.int32, device="cuda")[::2]):
        with pytest.raises(ValueError):
            m.sample_range(ctx, co4, t2, 0.0, 0.5, S, 5, valid=bad_valid)
    res, res_nv = m.sample_range(ctx, co4, t2, 0.0, 0.5, S, 5, out=good[: bsz * S * 15], valid=nv)
    ctx.sync()
    assert res.shape == (bsz, S, 5, 3) and res.data_ptr() == good.data_ptr() and res_nv.data_ptr() == nv.data_ptr()
