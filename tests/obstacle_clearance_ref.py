"""Independent reference of the sphere-obstacle clearance check (csrc/mtg_obstacle_lane.h): the smallest
||p(t) - c|| - r - inflation over [0, T] of one segment against one sphere -- plus the seeded inputs that
tests/test_obstacle_clearance.py and tests/test_gpu_obstacle_clearance.py share.  A plain module, pure numpy.

Method, per (segment, sphere):
  1. s(t) = sum_dim (p_dim(t) - c_dim)^2 is formed in np.longdouble by a plain double loop (no library convolution).
  2. Candidate times: 0, T, and for every numpy.roots(s') root with real part in [0, T] and |Im| <= 1e-3 T its real part as numpy
     gives it AND that value after three Newton steps on s' in np.longdouble (kept where it stays inside [0, T]).  The cut on the
     imaginary part is generous on purpose: a surplus candidate is a value of the same function and cannot hurt a minimum.
  3. The result is the smallest distance over the candidates, evaluated in np.longdouble from p - c by power sums (not from s,
     whose coefficients cancel, and not by the library's Horner recurrence), less r and the inflation.
Every candidate value is a value of the true function at a point of the interval, so the reference never falls below the true
minimum by more than its own rounding.  How complete it is cannot be argued, only tested: grid_min() is a 2001-point grid per
(segment, sphere), and the test module holds the reference to it.

Nothing here uses csrc/mtg_extrema_lane.h, oracle/ or the reference project's Jenkins-Traub.
"""
import math

import numpy as np

assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no wider than float64 on this platform"

LD = np.longdouble
IMAG_CUT = 1e-3
GRID = 2001


def distance(c, centre, t):
    """||p(t) - centre|| over dimensions 0-2 in longdouble by power sums; c [D][N], t [m] -> [m]."""
    t = np.atleast_1d(np.asarray(t, dtype=LD))
    a = np.asarray(c, dtype=np.float64)[:3].astype(LD).copy()
    a[:, 0] -= np.asarray(centre, dtype=np.float64).astype(LD)
    n = a.shape[1]
    pw = np.ones((len(t), n), dtype=LD)
    for e in range(1, n):
        pw[:, e] = pw[:, e - 1] * t
    r = (a[None, :, :] * pw[:, None, :]).sum(axis=2)
    return np.sqrt((r * r).sum(axis=1))


def candidate_times(c, centre, T):
    a = np.asarray(c, dtype=np.float64)[:3].astype(LD).copy()
    a[:, 0] -= np.asarray(centre, dtype=np.float64).astype(LD)
    n = a.shape[1]
    s = np.zeros(2 * n - 1, dtype=LD)
    for d in range(3):
        for i in range(n):
            for j in range(n):
                s[i + j] += a[d, i] * a[d, j]
    ds = s[1:] * np.arange(1, len(s), dtype=LD)
    cand = [LD(0.0), LD(T)]
    if not (T > 0.0):
        return np.array(cand, dtype=LD)
    f64 = ds.astype(np.float64)
    while len(f64) > 1 and f64[-1] == 0.0:
        f64 = f64[:-1]
    if len(f64) < 2 or not np.isfinite(f64).all():
        return np.array(cand, dtype=LD)
    roots = np.roots(f64[::-1] / np.abs(f64).max())
    keep = roots[(roots.real >= 0.0) & (roots.real <= T) & (np.abs(roots.imag) <= IMAG_CUT * T)].real
    cand += [LD(v) for v in keep]
    if keep.size:
        dds = ds[1:] * np.arange(1, len(ds), dtype=LD)
        x = keep.astype(LD)
        for _ in range(3):
            f = np.zeros_like(x)
            for v in ds[::-1]:
                f = f * x + v
            df = np.zeros_like(x)
            for v in dds[::-1]:
                df = df * x + v
            with np.errstate(divide="ignore", invalid="ignore"):
                x = x - np.where(df != 0, f / df, 0)
        cand += [v for v in x[np.isfinite(x) & (x >= 0) & (x <= LD(T))]]
    return np.array(cand, dtype=LD)


def pair_clearance(c, T, sphere, inflation=0.0):
    """(clearance, local time of the candidate that attains it) of one segment against one sphere (cx, cy, cz, r)."""
    t = candidate_times(c, sphere[:3], T)
    d = distance(c, sphere[:3], t)
    i = int(np.argmin(d))
    return d[i] - LD(sphere[3]) - LD(inflation), float(t[i])


def grid_min(coeffs, times, obstacles, inflation=0.0, points=GRID):
    """[B][K][M] float64: the smallest clearance on a grid of `points` per (segment, sphere), obstacles [M][4]."""
    tau = np.linspace(0.0, 1.0, points)
    t = times[:, :, None, None] * tau                                   # [B][K][1][P]
    val = np.zeros(times.shape + (3, points))
    for i in range(coeffs.shape[-1] - 1, -1, -1):
        val = val * t + coeffs[:, :, :3, i:i + 1]
    diff = val[:, :, None, :, :] - obstacles[None, None, :, :3, None]   # [B][K][M][3][P]
    return np.sqrt((diff * diff).sum(axis=3)).min(axis=3) - obstacles[:, 3] - inflation


def position_scale(coeffs, times):
    """[B]: max over the trajectory's segments of ||p(t)|| over dimensions 0-2 (on 65 points; the bounds need its size only)."""
    tau = np.linspace(0.0, 1.0, 65)
    t = times[:, :, None, None] * tau
    val = np.zeros(times.shape + (3, tau.size))
    for i in range(coeffs.shape[-1] - 1, -1, -1):
        val = val * t + coeffs[:, :, :3, i:i + 1]
    return np.sqrt((val * val).sum(axis=2)).max(axis=(1, 2))


def scale_of(coeffs, times, obstacles, inflation=0.0):
    """[B][M]: r + inflation + ||c|| + max ||p|| over the trajectory's segments, the size every bound here is relative to;
    obstacles [M][4] or [B][M][4]."""
    return obstacles[..., 3] + inflation + np.sqrt((obstacles[..., :3] ** 2).sum(axis=-1)) + position_scale(coeffs, times)[:, None]


# ---- the shared inputs ---------------------------------------------------------------------------------------------------
B, K, M = 13, 5, 8    # 65 lanes: one full 64-lane workgroup and one lane; the last trajectory's atomics come from two workgroups
SHAPES = [(n, d) for d in (3, 4) for n in range(4, 13)]
FAMILIES = ("far", "through", "waypoint")
CASES = [(n, d, f) for f in FAMILIES for n, d in SHAPES]


def seed_of(n, d, family):
    return 20261000 + 100 * n + d + 50 * FAMILIES.index(family)      # fixed before any result of the code under test was looked at


def make_inputs(n, d, family):
    """(coeffs [B][K][D][N], times [B][K], obstacles [M][4]).  Segment times uniform in [0.5, 3], coefficient i = 3 normal / i!
    (curves a few units long).  Spheres:
      'far'       centres 50 to 100 away from the origin, radii 1 to 5: nothing fails, every lower bound is far above zero;
      'through'   centres ON the curve of a seeded (trajectory, segment) at a seeded interior time, radii 0.3 to 1: that segment's
                  clearance is -r at an interior candidate;
      'waypoint'  sphere m centred on the START of segment (m, m mod K), radii 0.3 to 1: p(0) - c is exactly zero there and the
                  clearance exactly -r at a segment end."""
    rng = np.random.default_rng(seed_of(n, d, family))
    fact = np.array([math.factorial(i) for i in range(n)], dtype=np.float64)
    times = rng.uniform(0.5, 3.0, size=(B, K))
    coeffs = 3.0 * rng.standard_normal((B, K, d, n)) / fact
    obstacles = np.zeros((M, 4))
    if family == "far":
        v = rng.standard_normal((M, 3))
        obstacles[:, :3] = v / np.sqrt((v * v).sum(axis=1, keepdims=True)) * rng.uniform(50.0, 100.0, size=(M, 1))
        obstacles[:, 3] = rng.uniform(1.0, 5.0, size=M)
    else:
        obstacles[:, 3] = rng.uniform(0.3, 1.0, size=M)
        for m in range(M):
            if family == "waypoint":
                obstacles[m, :3] = coeffs[m, m % K, :3, 0]
            else:
                b, k = int(rng.integers(B)), int(rng.integers(K))
                t = rng.uniform(0.2, 0.8) * times[b, k]
                obstacles[m, :3] = [np.polyval(coeffs[b, k, dd, ::-1], t) for dd in range(3)]
    return np.ascontiguousarray(coeffs), np.ascontiguousarray(times), obstacles


_cache = {}


def reference(n, d, family):
    """{'coeffs', 'times', 'obstacles', 'pair' [B][K][M] longdouble clearances, 'pair_time' [B][K][M], 'scale' [B][M]}.  Computed
    once per case and shared; the arrays are read-only."""
    key = (n, d, family)
    if key not in _cache:
        coeffs, times, obstacles = make_inputs(n, d, family)
        pair = np.zeros((B, K, M), dtype=LD)
        pair_time = np.zeros((B, K, M))
        for b in range(B):
            for k in range(K):
                for m in range(M):
                    pair[b, k, m], pair_time[b, k, m] = pair_clearance(coeffs[b, k], times[b, k], obstacles[m])
        scale = scale_of(coeffs, times, obstacles)
        for a in (coeffs, times, obstacles, pair, pair_time, scale):
            a.setflags(write=False)
        _cache[key] = dict(coeffs=coeffs, times=times, obstacles=obstacles, pair=pair, pair_time=pair_time, scale=scale)
    return _cache[key]
