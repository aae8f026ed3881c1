"""Vectorised high-precision reference of mtg_sample_range (include/mtg_hip.h), pure numpy.

The choices a float64 caller can reproduce are made in float64 exactly as the header defines them (sample time t_i with two
roundings, sequential prefix sums of the segment times, the segment on the right of a vertex, seg_start = the prefix sum before
the segment's own time, local = min(t - seg_start, T_seg)); the polynomial and its derivatives are then evaluated in
np.longdouble by POWER SUMS with falling-factorial weights -- on purpose not the joint Horner recurrence of the kernels.

Pinned on the CPU (tests/test_oracle.py) against oracle_np.sample_batch (the line-cited restatement of the reference) and
against mpmath at 50 digits."""
import numpy as np

# 64-bit significand (x87 extended) or better: the reference must be ~2^-11 finer than the float64 bound it judges
assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no wider than float64 on this platform"


def sample_times(t_start, dt, n_samples):
    """t_i = fl(t_start + fl(i * dt)) in float64: two roundings (numpy never fuses)."""
    step = np.float64(dt) * np.arange(n_samples, dtype=np.float64)
    return np.float64(t_start) + step


def falling_factorial(n_coeffs, n_derivatives):
    """w[m][j] = j (j-1) ... (j-m+1) = m! C(j, m) (0 for j < m): d^m/dt^m t^j = w[m][j] t^(j-m)."""
    w = np.zeros((n_derivatives, n_coeffs), dtype=np.longdouble)
    for m in range(n_derivatives):
        for j in range(m, n_coeffs):
            v = 1
            for i in range(m):
                v *= j - i
            w[m, j] = v
    return w


def locate(times, t, b_idx):
    """(segment, local time) of sample times t [n] on trajectories b_idx [n]; times [B][K] float64."""
    times = np.ascontiguousarray(times, dtype=np.float64)
    k = times.shape[1]
    cum = np.cumsum(times, axis=1)                                   # sequential float64 accumulation
    c = cum[b_idx]
    seg = np.minimum((c <= t[:, None]).sum(axis=1), k - 1)
    rows = np.arange(len(t))
    seg_start = np.where(seg > 0, c[rows, np.maximum(seg - 1, 0)], 0.0)
    local = np.minimum(t - seg_start, times[b_idx, seg])
    return seg, local


def sample_ref(coeffs, times, t_start, dt, n_samples, n_derivatives, pairs=None):
    """coeffs [B][K][D][N], times [B][K] (float64) -> (want, scale, n_valid, seg, local).
    pairs = (b_idx, s_idx): only these (trajectory, sample) pairs, results [n][ND][D]; None: all, [B][S][ND][D].
    want   longdouble: derivatives 0..ND-1
    scale  float64: p~_m = m! sum_j C(j, m) |c_j| |local|^(j-m), the magnitude any evaluation error is relative to
    n_valid [B] int32: #{i : t_i <= total time} (always of the whole grid)."""
    coeffs = np.asarray(coeffs, dtype=np.float64)
    times = np.asarray(times, dtype=np.float64)
    bsz, k, dim, n = coeffs.shape
    assert times.shape == (bsz, k)
    tgrid = sample_times(t_start, dt, n_samples)
    total = np.cumsum(times, axis=1)[:, -1]
    n_valid = (tgrid[None, :] <= total[:, None]).sum(axis=1).astype(np.int32)
    if pairs is None:
        b_idx = np.repeat(np.arange(bsz), n_samples)
        s_idx = np.tile(np.arange(n_samples), bsz)
    else:
        b_idx, s_idx = (np.asarray(p, dtype=np.int64) for p in pairs)
    seg, local = locate(times, tgrid[s_idx], b_idx)
    c = coeffs[b_idx, seg].astype(np.longdouble)                     # [n][D][N]
    x = local.astype(np.longdouble)
    pw = np.ones((len(x), n), dtype=np.longdouble)                   # pw[:, e] = local^e
    for e in range(1, n):
        pw[:, e] = pw[:, e - 1] * x
    w = falling_factorial(n, n_derivatives)
    want = np.zeros((len(x), n_derivatives, dim), dtype=np.longdouble)
    scale = np.zeros((len(x), n_derivatives, dim), dtype=np.longdouble)
    for m in range(n_derivatives):
        if m >= n:
            continue
        terms = c[:, :, m:] * (w[m, m:][None, None, :] * pw[:, None, :n - m])
        want[:, m, :] = terms.sum(axis=2)
        scale[:, m, :] = np.abs(terms).sum(axis=2)
    scale = scale.astype(np.float64)
    if pairs is None:
        shape = (bsz, n_samples, n_derivatives, dim)
        want, scale = want.reshape(shape), scale.reshape(shape)
        seg, local = seg.reshape(bsz, n_samples), local.reshape(bsz, n_samples)
    return want, scale, n_valid, seg, local
