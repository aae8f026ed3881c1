"""CPU pins of tests/sampling_ref.py (the longdouble reference tests/test_gpu_sampling.py judges mtg_sample_range by):
against oracle_np.sample_batch, the line-cited restatement of Trajectory::evaluate / Polynomial::evaluate, against mpmath at
50 digits, and -- for the segment choice -- against integer arithmetic on a grid where every time is exact."""
import numpy as np

import sampling_ref as sr
from oracle import oracle_np as onp

U = 2.0 ** -53


def random_case(rng, bsz, k, dim, n, dyadic):
    # independent coefficients per segment over six decades: neighbouring segments are discontinuous
    coeffs = rng.standard_normal((bsz, k, dim, n)) * 10.0 ** rng.uniform(-3, 3, (bsz, k, dim, n))
    times = rng.integers(3, 25, (bsz, k)) * 0.125 if dyadic else rng.uniform(0.3, 3.0, (bsz, k))
    return coeffs, times


def test_reference_matches_the_restated_reference_loop():
    """sampling_ref.sample_ref == oracle_np.sample_batch to float64 Horner rounding, n_valid exactly.
    Bound per value: onp evaluates derivative m by one float64 Horner loop over pre-multiplied coefficients (<= N multiplies,
    N adds, N coefficient products): within (2N + ND + 2) u p~_m like any float64 evaluation (the bound of the GPU test).
    Shape 2 has inexact times; there onp's seg_start is fl(fl(acc + T) - T) (src/trajectory.cpp:66) and the header's is acc:
    they differ by delta <= 2 u total, which moves the value by delta |p^(m+1)| <= delta p~_(m+1) (second order ~1e-31 ignored;
    a factor 2 covers it)."""
    rng = np.random.default_rng(20240611)
    for (bsz, k, dim, n, S, nd, dyadic, t0, dt) in [(5, 4, 3, 10, 40, 5, True, -0.5, 0.25),
                                                    (4, 3, 2, 7, 33, 3, False, -0.3, 0.301)]:
        coeffs, times = random_case(rng, bsz, k, dim, n, dyadic)
        want, scale, nv, _, _ = sr.sample_ref(coeffs, times, t0, dt, S, nd + 1)
        got, got_nv = onp.sample_batch(coeffs, times, t0, dt, S, nd)
        assert np.array_equal(nv, got_nv)
        assert nv.min() >= 1 and nv.max() < S                 # samples before 0 and past the end are in the comparison
        bound = (2 * n + nd + 2) * U * scale[:, :, :nd]
        if not dyadic:
            total = times.sum(axis=1)[:, None, None, None]
            bound = bound + 4 * U * total * scale[:, :, 1:nd + 1]
        err = np.abs(got.astype(np.longdouble) - want[:, :, :nd]).astype(np.float64)
        assert (err <= bound).all(), float((err / bound).max())


def test_reference_matches_mpmath_at_50_digits():
    """The longdouble power sums against exact rational arithmetic (mpmath, 50 digits) on 360 samples.
    Bound: powers local^e carry <= (e - 1) roundings, each term two more products, the sum <= N - 1 additions:
    (2N + 2) u_l p~_m with u_l the unit round-off of np.longdouble."""
    import mpmath
    mpmath.mp.dps = 50
    ul = 2.0 ** -(np.finfo(np.longdouble).nmant + 1)
    rng = np.random.default_rng(7)
    worst = 0.0
    for (bsz, k, dim, n, S, nd) in [(3, 3, 2, 12, 20, 5), (3, 4, 1, 10, 20, 5), (3, 2, 3, 6, 20, 4), (3, 1, 2, 2, 20, 2)]:
        coeffs, times = random_case(rng, bsz, k, dim, n, False)
        want, scale, _, seg, local = sr.sample_ref(coeffs, times, -0.2, 0.23, S, nd)
        b_idx, s_idx = np.repeat(np.arange(bsz), S)[::2], np.tile(np.arange(S), bsz)[::2]     # 30 samples x nd x dim each
        for b, s in zip(b_idx, s_idx):
            x = mpmath.mpf(float(local[b, s]))
            for m in range(nd):
                for d in range(dim):
                    exact = mpmath.mpf(0)
                    for j in range(m, n):
                        exact += mpmath.ff(j, m) * mpmath.mpf(float(coeffs[b, seg[b, s], d, j])) * x ** (j - m)
                    w = want[b, s, m, d]
                    hi = float(w)
                    lo = float(w - np.longdouble(hi))
                    err = abs(mpmath.mpf(hi) + mpmath.mpf(lo) - exact)
                    bound = (2 * n + 2) * ul * scale[b, s, m, d]
                    assert err <= bound, (n, m, float(err), bound)
                    if bound > 0:
                        worst = max(worst, float(err / bound))
    assert worst > 0            # the comparison saw rounding at all (not identically zero operands)


def test_segment_choice_on_an_exact_grid():
    """Times and sample grid in multiples of 1/8: the header's rules in integer arithmetic -- a sample on a vertex belongs to the
    segment on its right at local time 0, the end time to the last segment at its end, later samples too, negative times to
    segment 0 with a negative local time."""
    rng = np.random.default_rng(3)
    units = rng.integers(1, 9, (6, 5))
    times = units * 0.125
    S, t0u, dtu = 60, -4, 1
    tgrid = sr.sample_times(t0u * 0.125, dtu * 0.125, S)
    assert np.array_equal(tgrid, (t0u + dtu * np.arange(S)) * 0.125)
    for b in range(6):
        seg, local = sr.locate(times, tgrid, np.full(S, b))
        ends = np.cumsum(units[b])
        hit = 0
        for s in range(S):
            tu = t0u + dtu * s
            k = int(np.searchsorted(ends, tu, side="right"))           # first segment whose end exceeds t
            k = min(k, 4)
            start = 0 if k == 0 else ends[k - 1]
            assert seg[s] == k and local[s] == min(tu - start, units[b, k]) * 0.125
            hit += tu in ends
        assert hit == 5
    _, _, nv, _, _ = sr.sample_ref(np.zeros((6, 5, 1, 2)), times, t0u * 0.125, dtu * 0.125, S, 1)
    assert np.array_equal(nv, np.minimum(units.sum(axis=1) - t0u + 1, S))
