"""Independent reference of the keep-out zone check (csrc/mtg_keepout_lane.h): the smallest over [0, T] of
max_j (offset_j - n_j . p(t)) - inflation of one segment against one zone of P planes -- plus the seeded inputs that
tests/test_keep_out.py and tests/test_gpu_keep_out.py share.  A plain module, pure numpy.

Method, per (segment, zone):
  1. Candidate times: 0, T, and the roots of every h_j' (one per distinct normal up to sign) and of every h_i - h_j (i < j, normals
     not equal): the projected polynomial is formed in float64, numpy.roots finds its roots, and every root with real part in
     [0, T] and |Im| <= 1e-3 T enters with its real part as numpy gives it AND with that value after three Newton steps in
     np.longdouble (kept where it stays inside [0, T]).  The cut on the imaginary part is generous on purpose: a surplus
     candidate is a value of the same function and cannot hurt a minimum.
  2. The result is the smallest envelope value over the candidates, evaluated in np.longdouble from p(t) by power sums (not by
     the library's Horner recurrence, not on the projected polynomials).
Every candidate value is a value of the true function at a point of the interval, so the reference never falls below the true
minimum by more than its own rounding.  How complete it is cannot be argued, only tested: grid_min() is a 2001-point grid per
(segment, zone), and the test module holds the reference to it.

Nothing here uses csrc/mtg_extrema_lane.h, oracle/ or the reference project's Jenkins-Traub.
"""
import math

import numpy as np

assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no wider than float64 on this platform"

LD = np.longdouble
IMAG_CUT = 1e-3
GRID = 2001
END, STATIONARY, PAIR = 0, 1, 2   # what kind of candidate attains a minimum


def position(c, t):
    """p(t) over dimensions 0-2 in longdouble by power sums; c [D][N], t [m] -> [m][3]."""
    t = np.atleast_1d(np.asarray(t, dtype=LD))
    a = np.asarray(c, dtype=np.float64)[:3].astype(LD)
    n = a.shape[1]
    pw = np.ones((len(t), n), dtype=LD)
    for e in range(1, n):
        pw[:, e] = pw[:, e - 1] * t
    return (a[None, :, :] * pw[:, None, :]).sum(axis=2)


def envelope(c, zone, t):
    """max_j (offset_j - n_j . p(t)) in longdouble; zone [P][4], t [m] -> [m]."""
    z = np.asarray(zone, dtype=np.float64).astype(LD)
    x = position(c, t)
    return (z[None, :, 3] - (x[:, None, :] * z[None, :, :3]).sum(axis=2)).max(axis=1)


def _roots_in(poly, T):
    """Candidates in [0, T] from the real roots of poly (increasing powers, longdouble): numpy's and the Newton-polished."""
    f64 = poly.astype(np.float64)
    while len(f64) > 1 and f64[-1] == 0.0:
        f64 = f64[:-1]
    if len(f64) < 2 or not np.isfinite(f64).all():
        return []
    roots = np.roots(f64[::-1] / np.abs(f64).max())
    keep = roots[(roots.real >= 0.0) & (roots.real <= T) & (np.abs(roots.imag) <= IMAG_CUT * T)].real
    out = [LD(v) for v in keep]
    if keep.size:
        dpoly = poly[1:] * np.arange(1, len(poly), dtype=LD)
        x = keep.astype(LD)
        for _ in range(3):
            f = np.zeros_like(x)
            for v in poly[::-1]:
                f = f * x + v
            df = np.zeros_like(x)
            for v in dpoly[::-1]:
                df = df * x + v
            with np.errstate(divide="ignore", invalid="ignore"):
                x = x - np.where(df != 0, f / df, 0)
        out += [v for v in x[np.isfinite(x) & (x >= 0) & (x <= LD(T))]]
    return out


def candidate_times(c, zone, T):
    """(times [m] longdouble, kinds [m]): 0, T, the stationary points of every h_j and the crossings of every pair."""
    a = np.asarray(c, dtype=np.float64)[:3].astype(LD)
    z = np.asarray(zone, dtype=np.float64)
    times, kinds = [LD(0.0), LD(T)], [END, END]
    if not (T > 0.0):
        return np.array(times, dtype=LD), np.array(kinds)
    zl = z.astype(LD)
    seen = []
    for j in range(len(z)):
        nj = tuple(z[j, :3])
        if any(nj == s or tuple(-v for v in nj) == s for s in seen):      # (tuples compare by value: +0 equals -0)
            continue
        seen.append(nj)
        q = (zl[j, :3, None] * a).sum(axis=0)
        found = _roots_in(q[1:] * np.arange(1, len(q), dtype=LD), T)
        times += found
        kinds += [STATIONARY] * len(found)
    for i in range(len(z)):
        for j in range(i + 1, len(z)):
            if tuple(z[i, :3]) == tuple(z[j, :3]):
                continue
            d = ((zl[j, :3] - zl[i, :3])[:, None] * a).sum(axis=0)       # h_i - h_j = (offset_i - offset_j) + (n_j - n_i) . p
            d[0] += zl[i, 3] - zl[j, 3]
            found = _roots_in(d, T)
            times += found
            kinds += [PAIR] * len(found)
    return np.array(times, dtype=LD), np.array(kinds)


def zone_clearance(c, T, zone, inflation=0.0):
    """(clearance, local time of the candidate that attains it, its kind, the smallest value over the END and STATIONARY
    candidates alone) of one segment against one zone."""
    t, kinds = candidate_times(c, zone, T)
    v = envelope(c, zone, t) - LD(inflation)
    i = int(np.argmin(v))
    return v[i], float(t[i]), int(kinds[i]), v[kinds != PAIR].min()


def _positions(coeffs, times, points):
    tau = np.linspace(0.0, 1.0, points)
    t = times[:, :, None, None] * tau                                   # [B][K][1][G]
    val = np.zeros(times.shape + (3, points))
    for i in range(coeffs.shape[-1] - 1, -1, -1):
        val = val * t + coeffs[:, :, :3, i:i + 1]
    return val                                                          # [B][K][3][G]


def grid_min(coeffs, times, zones, inflation=0.0, points=GRID):
    """[B][K][M] float64: the smallest clearance on a grid of `points` per (segment, zone), zones [M][P][4]."""
    val = _positions(coeffs, times, points)
    h = zones[None, None, :, :, 3, None] - np.einsum("mpd,bkdg->bkmpg", zones[:, :, :3], val)
    return h.max(axis=3).min(axis=3) - inflation


def speed_bound(coeffs, times):
    """[B][K]: an upper bound of ||p'(t)|| over [0, T]: sum_i i |p_i| T^(i-1), summed over the axes in the 2-norm."""
    n = coeffs.shape[-1]
    i = np.arange(1, n)
    per_axis = (np.abs(coeffs[:, :, :3, 1:]) * i * np.maximum(times, 0.0)[:, :, None, None] ** (i - 1)).sum(axis=3)
    return np.sqrt((per_axis ** 2).sum(axis=2))


def position_scale(coeffs, times):
    """[B]: max over the trajectory's segments of ||p(t)|| over dimensions 0-2 (on 65 points; the bounds need its size only)."""
    val = _positions(coeffs, times, 65)
    return np.sqrt((val * val).sum(axis=2)).max(axis=(1, 2))


def scale_of(coeffs, times, zones, inflation=0.0):
    """[B][M]: max_j |offset_j| + inflation + max ||p|| over the trajectory's segments, the size every bound here is relative
    to; zones [M][P][4] or [B][M][P][4]."""
    return np.abs(zones[..., 3]).max(axis=-1) + inflation + position_scale(coeffs, times)[:, None]


def oriented_box(centre, size, rotation=None):
    """[6][4]: the box with half sizes size / 2 along the columns of `rotation` (identity: bounding_box_half_planes' planes,
    order and signs): per axis the minimum face with +r, then the maximum face with -r."""
    r = np.eye(3) if rotation is None else np.asarray(rotation)
    centre, size = np.asarray(centre, dtype=np.float64), np.asarray(size, dtype=np.float64)
    out = np.zeros((6, 4))
    for axis in range(3):
        e = r[:, axis]
        out[2 * axis, :3], out[2 * axis, 3] = e, np.dot(centre - size[axis] / 2.0 * e, e)
        out[2 * axis + 1, :3], out[2 * axis + 1, 3] = -e, -np.dot(centre + size[axis] / 2.0 * e, e)
    return out


# ---- the shared inputs ---------------------------------------------------------------------------------------------------
B, K, M, P = 13, 5, 8, 6   # 65 lanes: one full 64-lane workgroup and one lane; the last trajectory's atomics come from two workgroups
SHAPES = [(n, d) for d in (3, 4) for n in range(4, 13)]
FAMILIES = ("far", "through", "waypoint", "corner")
CASES = [(n, d, f) for f in FAMILIES for n, d in SHAPES]


def seed_of(n, d, family):
    return 20261100 + 100 * n + d + 25 * FAMILIES.index(family)      # fixed before any result of the code under test was looked at


def _rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q


def make_inputs(n, d, family):
    """(coeffs [B][K][D][N], times [B][K], zones [M][6][4], seeded [M][2]: the (trajectory, segment) a zone was placed on, or -1).
    Segment times uniform in [0.5, 3], coefficient i = 3 normal / i! (curves a few units long).  Zones are boxes; the odd ones
    are rotated by a seeded orthogonal matrix, the even ones axis-aligned:
      'far'       centres 50 to 100 away from the origin, sizes 1 to 5: nothing fails, every lower bound is far above zero;
      'through'   centred ON the curve of a seeded (trajectory, segment) at a seeded interior time, sizes 0.6 to 2: that segment
                  is inside by half the smallest size at an interior candidate;
      'waypoint'  box m centred on the START of segment (m, m mod K), sizes 0.6 to 2: the clearance there is minus half the
                  smallest size at a segment end, or lower inside;
      'corner'    a seeded (trajectory, segment) passes an EDGE of box m outside it: at the seeded interior time t* the curve is
                  outside two faces by the same delta (0.2 to 0.5), moving away from one and towards the other (their outward
                  normals are (w + v) / sqrt 2 and (w - v) / sqrt 2, v the direction of motion tilted by a seeded vector of
                  length 0.4 -- at most 24 degrees, so both signs hold -- and w a seeded unit vector across v), so the
                  envelope has its kink -- a root of h_i - h_j, where no h_j' vanishes -- there.  Every box of this family is
                  rotated."""
    rng = np.random.default_rng(seed_of(n, d, family))
    fact = np.array([math.factorial(i) for i in range(n)], dtype=np.float64)
    times = rng.uniform(0.5, 3.0, size=(B, K))
    coeffs = 3.0 * rng.standard_normal((B, K, d, n)) / fact
    zones = np.zeros((M, P, 4))
    seeded = np.full((M, 2), -1)
    at = lambda b, k, t, der=0: np.array([np.polyval(np.polyder(coeffs[b, k, dd, ::-1], der) if der else coeffs[b, k, dd, ::-1], t)
                                          for dd in range(3)])
    for m in range(M):
        rot = _rotation(rng) if m % 2 else None
        if family == "far":
            v = rng.standard_normal(3)
            zones[m] = oriented_box(v / np.linalg.norm(v) * rng.uniform(50.0, 100.0), rng.uniform(1.0, 5.0, 3), rot)
            continue
        size = rng.uniform(0.6, 2.0, 3)
        if family == "waypoint":
            seeded[m] = m, m % K
            zones[m] = oriented_box(coeffs[m, m % K, :3, 0], size, rot)
            continue
        b, k = int(rng.integers(B)), int(rng.integers(K))
        seeded[m] = b, k
        t = rng.uniform(0.2, 0.8) * times[b, k]
        if family == "through":
            zones[m] = oriented_box(at(b, k, t), size, rot)
            continue
        v = at(b, k, t, 1)
        v /= np.linalg.norm(v)
        tilt = rng.standard_normal(3)            # (v itself would put the box's third axis across the motion: h' = 0 at t* there)
        v = v + 0.4 * tilt / np.linalg.norm(tilt)
        v /= np.linalg.norm(v)
        w = np.cross(v, rng.standard_normal(3))
        w /= np.linalg.norm(w)
        a0, a1 = (w + v) / math.sqrt(2.0), (w - v) / math.sqrt(2.0)      # outward normals of the two faces
        frame = np.stack([-a0, -a1, np.cross(a0, a1)], axis=1)           # the box lies on the - a0, - a1 side of the point
        delta = rng.uniform(0.2, 0.5)
        centre = at(b, k, t) - (delta + size[0] / 2.0) * a0 - (delta + size[1] / 2.0) * a1
        zones[m] = oriented_box(centre, size, frame)
    return np.ascontiguousarray(coeffs), np.ascontiguousarray(times), zones, seeded


_cache = {}


def reference(n, d, family):
    """{'coeffs', 'times', 'zones', 'seeded', 'pair' [B][K][M] longdouble clearances, 'pair_time' [B][K][M], 'kind' [B][K][M],
    'no_pairs' [B][K][M] (the minimum without the h_i - h_j candidates), 'scale' [B][M]}.  Computed once per case and shared;
    the arrays are read-only."""
    key = (n, d, family)
    if key not in _cache:
        coeffs, times, zones, seeded = make_inputs(n, d, family)
        pair = np.zeros((B, K, M), dtype=LD)
        no_pairs = np.zeros((B, K, M), dtype=LD)
        pair_time = np.zeros((B, K, M))
        kind = np.zeros((B, K, M), dtype=np.int64)
        for b in range(B):
            for k in range(K):
                for m in range(M):
                    pair[b, k, m], pair_time[b, k, m], kind[b, k, m], no_pairs[b, k, m] = zone_clearance(coeffs[b, k], times[b, k], zones[m])
        scale = scale_of(coeffs, times, zones)
        for a in (coeffs, times, zones, seeded, pair, pair_time, kind, no_pairs, scale):
            a.setflags(write=False)
        _cache[key] = dict(coeffs=coeffs, times=times, zones=zones, seeded=seeded, pair=pair, pair_time=pair_time, kind=kind,
                           no_pairs=no_pairs, scale=scale)
    return _cache[key]
