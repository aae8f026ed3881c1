"""Independent oracle of the per-axis extrema (mtg_minmax_axes): candidates 0, T and the near-real numpy.roots of p^(q+1),
Newton-polished and evaluated in numpy longdouble; the value bound every comparison uses; a 2001-point grid that shows nothing
was missed; the three seeded coefficient families of the tests.  Shared by tests/test_axis_minmax.py and
tests/test_gpu_axis_minmax.py; pinned on mpmath at 60 digits by the former."""
import numpy as np

LD = np.longdouble
MAX_ORDER = 4
GRID = 2001


def ff(k, q):
    """k (k - 1) .. (k - q + 1)"""
    r = 1.0
    for i in range(q):
        r *= k - i
    return r


def derivative(c, q):
    """Coefficients (increasing powers, longdouble) of the q-th derivative along the last axis; at least one coefficient."""
    c = np.asarray(c, dtype=LD)
    n = c.shape[-1]
    if q >= n:
        return np.zeros(c.shape[:-1] + (1,), dtype=LD)
    return c[..., q:] * np.array([ff(k, q) for k in range(q, n)], dtype=LD)


def evaluate(c, q, t):
    """p^(q)(t) in longdouble; c [..., N], t broadcastable to c's leading axes."""
    d = derivative(c, q)
    t = np.asarray(t, dtype=LD)
    r = np.zeros(np.broadcast(d[..., 0], t).shape, dtype=LD)
    for i in range(d.shape[-1] - 1, -1, -1):
        r = r * t + d[..., i]
    return r


def scale(c, T, q):
    """S = sum_{k >= q} ff(k, q) |p_k| T^(k - q): what the evaluation of p^(q) on [0, T] sums.  c [..., N], T [...]."""
    return np.asarray(evaluate(np.abs(np.asarray(c, dtype=np.float64)), q, np.abs(T)), dtype=np.float64)


def bound(c, T, q):
    """The bound of every value comparison: 1e-9 * max(1, S)."""
    return 1e-9 * np.maximum(1.0, scale(c, T, q))


def bounds(coeffs, times, first, n):
    """[B][K][D][n] for coeffs [B][K][D][N], times [B][K]."""
    return np.stack([bound(coeffs, times[:, :, None], first + j) for j in range(n)], axis=-1)


def candidates(c, T, q):
    """0, T, then the near-real roots of p^(q+1) in [0, T] (ascending), polished by Newton in longdouble.  A near-real root that
    is no root adds a point of [0, T]: its value cannot lie outside the true extrema."""
    d1 = np.asarray(derivative(c, q + 1), dtype=np.float64)
    d1 = np.trim_zeros(d1, "b")
    out = [LD(0.0), LD(T)]
    if d1.size >= 2:
        f, df = derivative(c, q + 1), derivative(c, q + 2)
        inner = []
        for r in np.roots(d1[::-1]):
            if abs(r.imag) > 1e-6 * max(1.0, abs(r)):
                continue
            x = LD(r.real)
            for _ in range(6):
                fx = sum(f[i] * x ** i for i in range(f.size))
                dfx = sum(df[i] * x ** i for i in range(df.size))
                if dfx == 0 or not np.isfinite(fx / dfx):
                    break
                x = x - fx / dfx
            if 0.0 <= x <= T:
                inner.append(x)
        out += sorted(inner)
    return out


def row(c, T, q):
    """(t_min, v_min, t_max, v_max) of p^(q) over [0, T] by the rule of Polynomial::selectMinMaxFromCandidates, in longdouble."""
    c = np.asarray(c, dtype=LD)
    t_min = t_max = LD(0.0)
    v_min, v_max = LD(np.finfo(np.float64).max), LD(-np.finfo(np.float64).max)
    for t in candidates(c, T, q):
        v = evaluate(c, q, t)
        if v < v_min:
            t_min, v_min = t, v
        if v > v_max:
            t_max, v_max = t, v
    return np.array([t_min, v_min, t_max, v_max], dtype=LD)


def table(coeffs, times):
    """[B][K][D][orders][4] (longdouble) for q = 0 .. min(4, N - 1)."""
    bsz, k, dim, n = coeffs.shape
    orders = min(MAX_ORDER, n - 1) + 1
    out = np.zeros((bsz, k, dim, orders, 4), dtype=LD)
    for b in range(bsz):
        for s in range(k):
            for d in range(dim):
                for q in range(orders):
                    out[b, s, d, q] = row(coeffs[b, s, d], times[b, s], q)
    return out


def grid_extrema(coeffs, times, q):
    """(min, max) [B][K][D] of p^(q) on GRID points of [0, T], longdouble."""
    tau = np.linspace(0.0, 1.0, GRID).astype(LD)
    t = np.asarray(times, dtype=LD)[:, :, None, None] * tau                     # [B][K][1][GRID]
    v = evaluate(np.asarray(coeffs, dtype=LD)[:, :, :, None, :], q, t)          # [B][K][D][GRID]
    return v.min(axis=-1), v.max(axis=-1)


def check_table(got, coeffs, times, first, want=None, grid=None):
    """The checks every result gets.  got [B][K][D][n][4] for the orders first .. first + n - 1.  Values against `want`
    ([B][K][D][n][4], reference data or the oracle) within the bound, no row left out; every reported time inside [0, T] with
    p^(q)(t) equal to the reported value within the bound; nothing above the maximum or below the minimum on the grid.
    grid: a dict that keeps the grid extrema of these coefficients from one call to the next.  Returns the worst
    |got - want| / max(1, S)."""
    n = got.shape[3]
    bnd = bounds(coeffs, times, first, n)
    T = times[:, :, None]
    worst = 0.0
    for j in range(n):
        q = first + j
        g = got[:, :, :, j]
        assert np.isfinite(g).all(), q
        for col in (0, 2):
            assert ((g[..., col] >= 0.0) & (g[..., col] <= T)).all(), (q, col, float(g[..., col].min()), float((g[..., col] - T).max()))
            own = np.abs(evaluate(coeffs, q, g[..., col]) - g[..., col + 1])
            assert (own <= bnd[..., j]).all(), (q, col, float(own.max()))
        if grid is None or q not in grid:
            lo, hi = grid_extrema(coeffs, times, q)
            if grid is not None:
                grid[q] = (lo, hi)
        lo, hi = (lo, hi) if grid is None else grid[q]
        assert (g[..., 3] >= hi - bnd[..., j]).all() and (g[..., 1] <= lo + bnd[..., j]).all(), q
        if want is not None:
            for col in (1, 3):
                err = np.abs(g[..., col] - want[:, :, :, j, col]).astype(np.float64)
                assert (err <= bnd[..., j]).all(), (q, col, float(err.max()), float((err / bnd[..., j]).max()))
                worst = max(worst, float((err / (bnd[..., j] / 1e-9)).max()))
    return worst


# ---- coefficient families (seeded) ---------------------------------------------------------------------------------------------

def factorials(n):
    return np.cumprod(np.concatenate([[1.0], np.arange(1.0, n)]))[:n]


def family_taylor(rng, bsz, k, dim, n):
    """random Taylor-like coefficients: normal / k!"""
    return rng.standard_normal((bsz, k, dim, n)) * 1.5 / factorials(n), rng.uniform(0.5, 2.0, (bsz, k))


def family_sinusoid(rng, bsz, k, dim, n):
    """Taylor coefficients of a sin(w t + phi) about t = 0"""
    a, w, phi = rng.uniform(0.5, 3.0, (bsz, k, dim, 1)), rng.uniform(1.0, 4.0, (bsz, k, dim, 1)), rng.uniform(0, 2 * np.pi, (bsz, k, dim, 1))
    j = np.arange(n)
    return a * w ** j * np.sin(phi + j * np.pi / 2.0) / factorials(n), rng.uniform(0.5, 2.0, (bsz, k))


def family_all_roots_inside(rng, bsz, k, dim, n):
    """p' = a prod (t - r_i) with all N - 2 roots r_i inside (0, T), spread one per equal cell: every level of the derivative chain
    has its full count of roots inside (Rolle), so both root buffers fill to the last element."""
    times = rng.uniform(0.8, 1.6, (bsz, k))
    coeffs = np.zeros((bsz, k, dim, n))
    m = n - 2
    for b in range(bsz):
        for s in range(k):
            for d in range(dim):
                if m >= 1:
                    cells = (np.arange(m) + rng.uniform(0.25, 0.75, m)) / m * times[b, s]
                    dp = np.poly(cells)[::-1] * rng.uniform(0.5, 2.0) * rng.choice([-1.0, 1.0])   # increasing powers, degree m
                else:
                    dp = np.array([rng.standard_normal()])[:max(n - 1, 0)]
                coeffs[b, s, d, 0] = rng.standard_normal()
                coeffs[b, s, d, 1:1 + dp.size] = dp / np.arange(1, dp.size + 1)
    return coeffs, times


FAMILIES = {"taylor": family_taylor, "sinusoid": family_sinusoid, "all_roots_inside": family_all_roots_inside}


def valid_ranges(n):
    """every (first, count) with first + count - 1 <= min(4, N - 1)"""
    last = min(MAX_ORDER, n - 1)
    return [(f, c) for f in range(last + 1) for c in range(1, last - f + 2)]
