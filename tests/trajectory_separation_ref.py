"""Independent reference of the trajectory-to-trajectory separation check (csrc/mtg_separation_lane.h): the smallest
||pA(t) - pB(t)|| over the time two piecewise polynomial trajectories both fly -- plus the seeded inputs that
tests/test_trajectory_separation.py and tests/test_gpu_trajectory_separation.py share.  A plain module, pure numpy.

Method, per pair:
  1. Breakpoints by the library's rule: e[0] = start, e[i + 1] = e[i] + T[i], one float64 addition per step.  Pieces are all (i, j)
     with lo = max(ea[i], eb[j]) < hi = min(ea[i + 1], eb[j + 1]).
  2. Per piece, with x the time since lo: both polynomials are shifted to x in np.longdouble (binomial expansion, plain loops),
     subtracted, and s(x) = sum_dim d_dim(x)^2 is formed by a plain loop (no library convolution).
  3. Candidates: x = 0, x = L = hi - lo, and for every numpy.roots(s') root with real part in [0, L] and |Im| <= 1e-3 L its real
     part as numpy gives it AND that value after three Newton steps on s' in np.longdouble (kept where it stays inside [0, L]).
  4. Values come from the ORIGINAL two polynomials at their own local times (lo - ea[i]) + x and (lo - eb[j]) + x by power sums
     in np.longdouble, not from the shifted difference and not by a Horner recurrence.
Every candidate value is a value of the true function at a time both fly, so the reference never falls below the true minimum by
more than its own rounding.  How complete it is cannot be argued, only tested: grid_min() is a 2001-point grid per pair window,
and the test module holds the reference to it.

Nothing here uses csrc/, oracle/ or the reference project's Jenkins-Traub.
"""
import math

import numpy as np

assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no wider than float64 on this platform"

LD = np.longdouble
IMAG_CUT = 1e-3
GRID = 2001


def breakpoints(times, start=0.0):
    e = [np.float64(start)]
    for T in np.asarray(times, dtype=np.float64):
        e.append(np.float64(e[-1] + T))
    return np.array(e, dtype=np.float64)


def pieces(ea, eb):
    """[(i, j, lo, hi)] in time order."""
    out = []
    for i in range(len(ea) - 1):
        for j in range(len(eb) - 1):
            lo, hi = max(ea[i], eb[j]), min(ea[i + 1], eb[j + 1])
            if lo < hi:
                out.append((i, j, lo, hi))
    return sorted(out, key=lambda p: p[0] + p[1])


def _shift(c, s):
    """Coefficients of p(s + x) in x, longdouble; c [3][N] float64."""
    n = c.shape[1]
    out = np.zeros((3, n), dtype=LD)
    s = LD(s)
    for k in range(n):
        for i in range(k + 1):
            out[:, i] += LD(math.comb(k, i)) * c[:, k].astype(LD) * s ** (k - i)
    return out


def _value(c, t):
    """p(t) over dimensions 0-2 by power sums in longdouble; c [D][N], t [m] -> [m][3]."""
    a = np.asarray(c, dtype=np.float64)[:3].astype(LD)
    n = a.shape[1]
    pw = np.ones((len(t), n), dtype=LD)
    for e in range(1, n):
        pw[:, e] = pw[:, e - 1] * t
    return (a[None, :, :] * pw[:, None, :]).sum(axis=2)


def distance(ca, sa, cb, sb, x):
    """||pA(sa + x) - pB(sb + x)|| from the two originals; x [m] longdouble."""
    x = np.atleast_1d(np.asarray(x, dtype=LD))
    r = _value(ca, LD(sa) + x) - _value(cb, LD(sb) + x)
    return np.sqrt((r * r).sum(axis=1))


def candidate_times(ca, sa, cb, sb, L):
    d = _shift(np.asarray(ca, dtype=np.float64)[:3], sa) - _shift(np.asarray(cb, dtype=np.float64)[:3], sb)
    n = d.shape[1]
    s = np.zeros(2 * n - 1, dtype=LD)
    for k in range(3):
        for i in range(n):
            s[i:i + n] += d[k, i] * d[k]
    ds = s[1:] * np.arange(1, len(s), dtype=LD)
    cand = [LD(0.0), LD(L)]
    f64 = ds.astype(np.float64)
    while len(f64) > 1 and f64[-1] == 0.0:
        f64 = f64[:-1]
    if len(f64) < 2 or not np.isfinite(f64).all() or not np.abs(f64).max() > 0.0:
        return np.array(cand, dtype=LD)
    roots = np.roots(f64[::-1] / np.abs(f64).max())
    keep = roots[(roots.real >= 0.0) & (roots.real <= L) & (np.abs(roots.imag) <= IMAG_CUT * L)].real
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
        cand += [v for v in x[np.isfinite(x) & (x >= 0) & (x <= LD(L))]]
    return np.array(cand, dtype=LD)


def pair_pieces(ca, ta, start_a, cb, tb, start_b):
    """[(i, j, lo, hi, distance (longdouble), global time of the candidate that attains it)] of one pair, in time order; ca
    [Ka][D][N], ta [Ka]."""
    ea, eb = breakpoints(ta, start_a), breakpoints(tb, start_b)
    out = []
    for i, j, lo, hi in pieces(ea, eb):
        sa, sb, L = lo - ea[i], lo - eb[j], hi - lo
        x = candidate_times(ca[i], sa, cb[j], sb, L)
        d = distance(ca[i], sa, cb[j], sb, x)
        k = int(np.argmin(d))
        out.append((i, j, lo, hi, d[k], float(lo + float(x[k]))))
    return out


def fold(piece_list, ka, min_separation):
    """What the check reports for one pair from its pieces' distances: a dict with the pair's and the per-segment results
    (distances still WITHOUT min_separation subtracted: 'distance', 'segment_distance')."""
    seg_d = np.full(ka, np.inf, dtype=LD)
    seg_t = np.full(ka, np.nan)
    seg_b = np.full(ka, -1, dtype=np.int32)
    seg_n = np.zeros(ka, dtype=np.int32)
    best, best_t, best_a, best_b, first = LD(np.inf), np.nan, -1, -1, (-1, -1)
    runner_up = LD(np.inf)      # the smallest distance of a piece other than the best one
    for i, j, lo, hi, d, t in piece_list:
        seg_n[i] += 1
        if d < seg_d[i]:
            seg_d[i], seg_t[i], seg_b[i] = d, t, j
        if d < best:
            runner_up = best
            best, best_t, best_a, best_b = d, t, i, j
        elif d < runner_up:
            runner_up = d
        if first[0] < 0 and not (d - LD(min_separation) > 0):
            first = (i, j)
    return dict(distance=best, time=best_t, segment_a=best_a, segment_b=best_b, first=first, feasible=int(first[0] < 0),
                runner_up=runner_up, segment_distance=seg_d, segment_time=seg_t, segment_b_of=seg_b, segment_pieces=seg_n)


def _positions(c, t_local):
    val = np.zeros(t_local.shape + (3,))
    for i in range(c.shape[-1] - 1, -1, -1):
        val = val * t_local[..., None] + c[..., :3, i]
    return val


def grid_min(ca, ta, start_a, cb, tb, start_b, points=GRID):
    """The smallest distance on a grid of `points` global times over the pair's window (float64); +inf for an empty window."""
    ea, eb = breakpoints(ta, start_a), breakpoints(tb, start_b)
    lo, hi = max(ea[0], eb[0]), min(ea[-1], eb[-1])
    if not lo < hi:
        return np.inf
    t = np.linspace(lo, hi, points)
    ia = np.clip(np.searchsorted(ea, t, side="right") - 1, 0, len(ta) - 1)
    ib = np.clip(np.searchsorted(eb, t, side="right") - 1, 0, len(tb) - 1)
    pa = _positions(np.asarray(ca)[ia], t - ea[ia])
    pb = _positions(np.asarray(cb)[ib], t - eb[ib])
    return float(np.sqrt(((pa - pb) ** 2).sum(axis=1)).min())


def position_scale(coeffs, times):
    """[B]: max over the trajectory's segments of ||p(t)|| over dimensions 0-2 (on 65 points; the bounds need its size only)."""
    tau = np.linspace(0.0, 1.0, 65)
    t = times[:, :, None, None] * tau
    val = np.zeros(times.shape + (3, tau.size))
    for i in range(coeffs.shape[-1] - 1, -1, -1):
        val = val * t + coeffs[:, :, :3, i:i + 1]
    return np.sqrt((val * val).sum(axis=2)).max(axis=(1, 2))


def scale_of(coeffs_a, times_a, coeffs_b, times_b, pairs, min_separation=0.0):
    """[P]: min_separation + max ||pA|| + max ||pB|| over the two trajectories' segments, the size every bound here is relative to."""
    return min_separation + position_scale(coeffs_a, times_a)[pairs[:, 0]] + position_scale(coeffs_b, times_b)[pairs[:, 1]]


# ---- the shared inputs ---------------------------------------------------------------------------------------------------
BA, BB, P = 7, 6, 13   # with Ka = 5: 65 lanes, one full 64-lane workgroup and one lane
SHAPES = [(n, d) for d in (3, 4) for n in range(1, 13)]
FAMILIES = ("far", "crossing", "random")
MIN_SEPARATION = {"far": 1.0, "crossing": 0.5, "random": 1.5}
KS = {"far": (5, 4), "crossing": (5, 3), "random": (5, 7)}
CASES = [(n, d, f) for f in FAMILIES for n, d in SHAPES]


def seed_of(n, d, family, ka, kb):
    return 20261100 + 1000 * FAMILIES.index(family) + 40 * n + 10 * d + 3 * ka + kb   # fixed before any result was looked at


def make_inputs(n, d, family, ka=None, kb=None, ba=BA, bb=BB, n_pairs=P):
    """dict(coeffs_a [ba][ka][D][N], times_a [ba][ka], start_a [ba], coeffs_b, times_b, start_b, pairs [n_pairs][2] int32,
    min_separation).  Segment times uniform in [0.5, 3], starts uniform in [0, 1.5], coefficient i = 3 normal / i! (curves a few
    units long, every segment on its own: the curves jump at their breakpoints).  Side B:
      'far'       moved 50 to 100 away: nothing fails, every lower bound is far above the running minimum after the first piece;
      'crossing'  for each trajectory of B the first pair that names it: the segment of B that flies in the middle of the common
                  window is moved so that the two MEET there -- the separation is -min_separation at an interior candidate;
      'random'    as side A: both verdicts."""
    ka = KS[family][0] if ka is None else ka
    kb = KS[family][1] if kb is None else kb
    rng = np.random.default_rng(seed_of(n, d, family, ka, kb))
    fact = np.array([math.factorial(i) for i in range(n)], dtype=np.float64)
    ta, tb = rng.uniform(0.5, 3.0, size=(ba, ka)), rng.uniform(0.5, 3.0, size=(bb, kb))
    sa, sb = rng.uniform(0.0, 1.5, size=ba), rng.uniform(0.0, 1.5, size=bb)
    ca, cb = 3.0 * rng.standard_normal((ba, ka, d, n)) / fact, 3.0 * rng.standard_normal((bb, kb, d, n)) / fact
    pairs = np.stack([rng.integers(ba, size=n_pairs), rng.integers(bb, size=n_pairs)], axis=1).astype(np.int32)
    if family == "far":
        v = rng.standard_normal((bb, 3))
        cb[:, :, :3, 0] += (v / np.sqrt((v * v).sum(axis=1, keepdims=True)) * rng.uniform(50.0, 100.0, size=(bb, 1)))[:, None, :]
    if family == "crossing":
        seen = set()
        for a, b in pairs:
            if b in seen:
                continue
            seen.add(b)
            ea, eb = breakpoints(ta[a], sa[a]), breakpoints(tb[b], sb[b])
            lo, hi = max(ea[0], eb[0]), min(ea[-1], eb[-1])
            tg = lo + rng.uniform(0.35, 0.65) * (hi - lo)
            i = int(np.clip(np.searchsorted(ea, tg, side="right") - 1, 0, ka - 1))
            j = int(np.clip(np.searchsorted(eb, tg, side="right") - 1, 0, kb - 1))
            pa = np.array([np.polyval(ca[a, i, k, ::-1], tg - ea[i]) for k in range(3)])
            pb = np.array([np.polyval(cb[b, j, k, ::-1], tg - eb[j]) for k in range(3)])
            cb[b, j, :3, 0] += pa - pb
    return dict(coeffs_a=np.ascontiguousarray(ca), times_a=np.ascontiguousarray(ta), start_a=sa, coeffs_b=np.ascontiguousarray(cb),
                times_b=np.ascontiguousarray(tb), start_b=sb, pairs=np.ascontiguousarray(pairs), min_separation=MIN_SEPARATION[family])


_cache = {}


def reference_of(z):
    """The pieces of every pair of an input dict: [P] lists of pair_pieces()."""
    return [pair_pieces(z["coeffs_a"][a], z["times_a"][a], z["start_a"][a], z["coeffs_b"][b], z["times_b"][b], z["start_b"][b])
            for a, b in z["pairs"]]


def reference(n, d, family):
    """make_inputs(n, d, family) with 'pieces' (reference_of) and 'scale' [P].  Computed once per case and shared; the arrays are
    read-only."""
    key = (n, d, family)
    if key not in _cache:
        z = make_inputs(n, d, family)
        z["pieces"] = reference_of(z)
        z["scale"] = scale_of(z["coeffs_a"], z["times_a"], z["coeffs_b"], z["times_b"], z["pairs"], z["min_separation"])
        for v in z.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = z
    return _cache[key]
