"""Independent reference of the gradient with respect to the free derivatives (mtg_free_gradient), in mpmath at 50 digits.

It builds, per segment, A(T) literally from the derivative rows of the monomials at 0 and at T, inverts it in 50 digits, builds
Q(T) from its integral formula, and returns (A^-1 M)^T (G + w Q c) over all K + 1 vertices, split by the masks into the free and
the fixed columns.  It shares nothing with the lane code: no scaling identity, none of the committed tables.  Next to every
output it returns sum|terms|: the same expression with every factor and addend replaced by its absolute value."""
import functools

import mpmath as mp
import numpy as np

mp.mp.dps = 50


def falling(i, p):
    """i! / (i - p)!: the p-th derivative of t^i is falling(i, p) t^(i - p)."""
    out = 1
    for q in range(p):
        out *= i - q
    return out


@functools.lru_cache(maxsize=4096)
def a_inverse(N, T):
    """A(T)^-1, A rows 0 .. h-1: derivative p at 0, rows h .. N-1: derivative p at T (T a float, taken exactly)."""
    h = N // 2
    t = mp.mpf(T)
    A = mp.zeros(N, N)
    for p in range(h):
        A[p, p] = falling(p, p)
        for i in range(p, N):
            A[h + p, i] = falling(i, p) * t ** (i - p)
    return A ** -1


@functools.lru_cache(maxsize=4096)
def q_matrix(N, d, T):
    """Q(T)_ij = int_0^T 2 (t^i)^(d) (t^j)^(d) dt: the cost is 0.5 c^T Q c (computeCost, LIN:124-140)."""
    t = mp.mpf(T)
    Q = mp.zeros(N, N)
    for i in range(d, N):
        for j in range(d, N):
            e = i + j - 2 * d + 1
            Q[i, j] = mp.mpf(2 * falling(i, d) * falling(j, d)) * t ** e / e
    return Q


def columns(N, masks):
    """(vertex, derivative) -> ('fixed' | 'free', column) in the order of d_fixed / d_free, and the two counts."""
    h = N // 2
    col, nf, np_ = {}, 0, 0
    for v, m in enumerate(masks):
        for p in range(h):
            if (int(m) >> p) & 1:
                col[(v, p)] = ("fixed", nf)
                nf += 1
            else:
                col[(v, p)] = ("free", np_)
                np_ += 1
    return col, nf, np_


def pull_back_vertices(N, d, times, grad, coeffs, w):
    """One trajectory: times [K], grad / coeffs [K][D][N] or None -> (g, a): [D][K+1][h] lists of mpf, the pull-back onto every
    vertex derivative and its sum|terms|."""
    h, K = N // 2, len(times)
    D = (grad if grad is not None else coeffs).shape[1]
    g = [[[mp.mpf(0)] * h for _ in range(K + 1)] for _ in range(D)]
    a = [[[mp.mpf(0)] * h for _ in range(K + 1)] for _ in range(D)]
    wq = mp.mpf(w)
    for k in range(K):
        Ai = a_inverse(N, float(times[k]))
        Q = q_matrix(N, d, float(times[k])) if coeffs is not None else None
        for dim in range(D):
            G = [mp.mpf(float(grad[k, dim, i])) if grad is not None else mp.mpf(0) for i in range(N)]
            Ga = [abs(x) for x in G]
            if coeffs is not None:
                c = [mp.mpf(float(coeffs[k, dim, j])) for j in range(N)]
                for i in range(N):
                    G[i] += wq * mp.fsum(Q[i, j] * c[j] for j in range(N))
                    Ga[i] += abs(wq) * mp.fsum(abs(Q[i, j]) * abs(c[j]) for j in range(N))
            for r in range(N):        # row r of (A^-1)^T G: x_S,r for r < h, x_E,(r-h) beyond
                val = mp.fsum(Ai[i, r] * G[i] for i in range(N))
                av = mp.fsum(abs(Ai[i, r]) * Ga[i] for i in range(N))
                v, p = (k, r) if r < h else (k + 1, r - h)
                g[dim][v][p] += val
                a[dim][v][p] += av
    return g, a


def reference(N, d, masks, times, grad=None, coeffs=None, w=1.0):
    """Batch: times [B][K], grad / coeffs [B][K][D][N] or None.  Returns a dict of object arrays of mpf:
    free, abs_free [B][D][n_free];  fixed, abs_fixed [B][D][n_fixed];  vertices, abs_vertices [B][D][K+1][h]."""
    times = np.asarray(times, dtype=np.float64)
    B, K = times.shape
    h = N // 2
    src = grad if grad is not None else coeffs
    D = src.shape[2]
    col, n_fixed, n_free = columns(N, masks)
    out = {"free": np.empty((B, D, n_free), dtype=object), "abs_free": np.empty((B, D, n_free), dtype=object),
           "fixed": np.empty((B, D, n_fixed), dtype=object), "abs_fixed": np.empty((B, D, n_fixed), dtype=object),
           "vertices": np.empty((B, D, K + 1, h), dtype=object), "abs_vertices": np.empty((B, D, K + 1, h), dtype=object)}
    for b in range(B):
        g, a = pull_back_vertices(N, d, times[b], None if grad is None else grad[b], None if coeffs is None else coeffs[b], w)
        for dim in range(D):
            for v in range(K + 1):
                for p in range(h):
                    kind, c = col[(v, p)]
                    out[kind][b, dim, c] = g[dim][v][p]
                    out["abs_" + kind][b, dim, c] = a[dim][v][p]
                    out["vertices"][b, dim, v, p] = g[dim][v][p]
                    out["abs_vertices"][b, dim, v, p] = a[dim][v][p]
    return out


def forward_jacobian_apply(N, masks, times, d_free, d_fixed):
    """The forward map in 50 digits for one trajectory: d_free [D][n_free], d_fixed [D][n_fixed] -> coeffs [K][D][N] (mpf)."""
    h, K = N // 2, len(times)
    col, _, _ = columns(N, masks)
    D = len(d_free)
    out = np.empty((K, D, N), dtype=object)
    for k in range(K):
        Ai = a_inverse(N, float(times[k]))
        for dim in range(D):
            x = []
            for v in (k, k + 1):
                for p in range(h):
                    kind, c = col[(v, p)]
                    x.append(mp.mpf(float((d_fixed if kind == "fixed" else d_free)[dim][c])))
            for i in range(N):
                out[k, dim, i] = mp.fsum(Ai[i, r] * x[r] for r in range(N))
    return out


def to_float(a):
    return np.array([float(x) for x in a.ravel()], dtype=np.float64).reshape(a.shape)


def worst_share(got, ref, abs_ref, constant):
    """max over the entries of |got - ref| / (constant 2^-53 sum|terms|); an entry with sum|terms| = 0 must be exactly 0."""
    worst = 0.0
    e = mp.mpf(2) ** -53
    for x, r, s in zip(np.asarray(got).ravel(), ref.ravel(), abs_ref.ravel()):
        err = abs(mp.mpf(float(x)) - r)
        if s == 0:
            assert float(x) == 0.0
            continue
        worst = max(worst, float(err / (constant * e * s)))
    return worst
