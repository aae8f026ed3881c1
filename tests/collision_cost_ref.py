"""Independent reference of the distance-field collision cost and its gradient (include/mtg_hip.h, mtg_collision_cost): numpy,
longdouble, vectorised over all samples of a batch.  The sample TIMES and the trapezoid WEIGHTS follow the float64 rule of the
specification (they are part of it); everything after them is longdouble with plain sums: Horner p and v, u by a true division,
d and G from the float32 voxels as weighted sums, the potential, the speed, the terms.

reference() returns the cost and the gradient per segment, sum |term| per output, an a-priori bound per output and the fragile
samples.

The bound.  e = 2^-53; first order in e; every constant counts the roundings of the float64 path and is rounded up.  Per sample:
  dp_a  = e 2 N ptilde_a,  ptilde_a = sum_i |c_a,i| t^i           Horner's running bound, one fma per coefficient (the field
                                                                   check's derivation); with the two roundings of u:
  du_a  = e ((2 N + 4) ptilde_a + 2 |p_a - origin_a|) / h          distance_field_ref.py's own term
  dv_a  = e (2 N + 2) vtilde_a,  vtilde_a = sum_i i |c_a,i| t^(i-1)   every product c_i t^(i-1) of v passes through at most 2 N
                                                                   fused steps of the joint recurrence
  dd    = sum_a Gamma_a du_a + e 16 D_max                          Gamma_a = largest |difference| of neighbouring voxels along a:
                                                                   |dd/du_a| <= Gamma_a; 16 D_max: the seven interpolation steps
  dG_a  = (2 Gamma_a sum_{b != a} du_b + e (16 D_max + 8 Gamma_a)) / h
                                                                   G_a is bilinear in the other two u_b with slopes of at most a
                                                                   difference of two a-differences (2 Gamma_a); its own steps
                                                                   work on x**, y* that carry e D_max each, and on r = fl(1 / h)
  dx    = dd + e |x|                                               x = d - inflation
  dc    = dx + 4 e c                                               |c'| <= 1: c is 1-Lipschitz; sub, mul, div, fl(2 epsilon)
  dc'   = dx / epsilon + 3 e |c'|                                  c' is (1 / epsilon)-Lipschitz
  ds    = sum_a dv_a |v_a| / s + 4 e s                             |ds/dv_a| = |v_a| / s; three fma, fl(eta^2) and the root
  term  = w c s:            dterm = w (dc s + c ds) + 2 e |term|
  A_a   = w c' s G_a:       dA_a  = w (dc' s |G_a| + |c'| ds |G_a| + |c'| s dG_a) + 3 e |A_a|
  B_a   = w c v_a / s:      dB_a  = w (dc |v_a| / s + c sum_b dv_b / s) + 3 e |B_a|
                                                                   d(v / s)/dv = (I - v v^T / s^2) / s has norm <= 1 / s, and
                                                                   1 / s <= 1 / speed_epsilon: the bound is finite at rest
Per output, bound = bound_terms + bound_sum:
  cost:          sum_i dterm                           + e (S + 6) sum_i |term|
  entry (a, j):  sum_i (dA_a t^j + dB_a j t^(j-1))     + e (S + 6 + 2 j) sum_i (|A_a| t^j + |B_a| j t^(j-1))
(S + 6: no term passes through more additions than that, whatever the partition into partial sums; 2 j: the j - 1 products of
the power, the product with j, the fma).  Continuity carries the bound across the potential's two joints (c and c' are
continuous there, so a computed x on the other side of a joint changes them by no more than their Lipschitz bound); it does NOT
carry across an integer u_a, where G_a jumps: those samples are FRAGILE, as are samples next to a domain edge, where d and G jump
to outside_distance and 0.  Nothing here was tuned to the code under test."""
import numpy as np

import distance_field_ref as R

LD = np.longdouble
EPS = 2.0 ** -53


def weights(t, S, times):
    """w [B][K][Smax] float64 by the rule: fl(fl(t_{i+1} - t_{i-1}) 0.5) with both neighbours clamped to the segment; 0 beyond
    S and for T <= 0; NaN for a NaN T."""
    smax = t.shape[-1]
    i = np.arange(smax)
    last = (S - 1)[..., None]
    hi = np.take_along_axis(t, np.minimum(i + 1, last), axis=-1)
    lo = np.take_along_axis(t, np.broadcast_to(np.maximum(i - 1, 0), t.shape), axis=-1)
    with np.errstate(invalid="ignore"):
        w = (hi - lo) * 0.5
        w = np.where((times <= 0.0)[..., None], 0.0, w)
    return np.where(i <= last, w, 0.0)


def field_and_gradient(grid, u, h, outside):
    """d [...] and G [...][3] (longdouble) of the trilinear interpolant at voxel coordinates u [...][3]; outside: the value and 0;
    a NaN u_a: NaN."""
    nz, ny, nx = grid.shape
    n = np.array([nx, ny, nz])
    nan = np.isnan(u).any(axis=-1)
    u = np.where(np.isnan(u), 0, u)
    inside = ((u >= 0) & (u <= n - 1)).all(axis=-1)
    i = np.clip(np.floor(u), 0, n - 2).astype(np.int64)
    f = u - i
    g = grid.astype(LD)
    V = [[[g[i[..., 2] + dz, i[..., 1] + dy, i[..., 0] + dx] for dx in (0, 1)] for dy in (0, 1)] for dz in (0, 1)]
    wt = lambda a, hi: f[..., a] if hi else 1 - f[..., a]
    d = sum(wt(0, dx) * wt(1, dy) * wt(2, dz) * V[dz][dy][dx] for dx in (0, 1) for dy in (0, 1) for dz in (0, 1))
    gx = sum(wt(1, dy) * wt(2, dz) * (V[dz][dy][1] - V[dz][dy][0]) for dy in (0, 1) for dz in (0, 1))
    gy = sum(wt(0, dx) * wt(2, dz) * (V[dz][1][dx] - V[dz][0][dx]) for dx in (0, 1) for dz in (0, 1))
    gz = sum(wt(0, dx) * wt(1, dy) * (V[1][dy][dx] - V[0][dy][dx]) for dx in (0, 1) for dy in (0, 1))
    G = np.stack([gx, gy, gz], axis=-1) / LD(h)
    d, G = np.where(inside, d, LD(outside)), np.where(inside[..., None], G, LD(0))
    return np.where(nan, LD(np.nan), d), np.where(nan[..., None], LD(np.nan), G), inside & ~nan


def potential(x, epsilon):
    """The CHOMP potential c and c' (longdouble)."""
    e = LD(epsilon)
    with np.errstate(invalid="ignore"):
        c = np.where(x < 0, e / 2 - x, np.where(x <= e, (x - e) ** 2 / (2 * e), LD(0)))
        dc = np.where(x < 0, LD(-1), np.where(x <= e, (x - e) / e, LD(0)))
    return np.where(np.isnan(x), LD(np.nan), c), np.where(np.isnan(x), LD(np.nan), dc)


def reference(coeffs, times, grid, origin, h, outside, dt, inflation, epsilon, speed_epsilon, want_terms=False):
    """dict: S [B][K]; cost, abs_cost (sum |term|), bound_cost, bound_terms_cost [B][K]; grad, abs_grad, bound_grad,
    bound_terms_grad [B][K][3][N]; fragile [B][K][Smax]; u_gap (the smallest distance of an inside sample's u_a to an integer);
    positive (samples with c > 0), samples (valid ones).  want_terms: also terms [B][K][Smax] and grad_terms [B][K][Smax][3][N]
    rounded to float64, w, t, valid.  coeffs may be longdouble (the central-difference test perturbs them below float64)."""
    c = np.asarray(coeffs)[:, :, :3, :].astype(LD)                    # [B][K][3][N]
    times = np.asarray(times, dtype=np.float64)
    t, valid, S = R.sample_times(times, dt)
    w = weights(t, S, times)
    N = c.shape[-1]
    tl = t.astype(LD)[:, :, :, None]                                  # [B][K][Smax][1]
    p = np.zeros(t.shape + (3,), dtype=LD)
    v = np.zeros_like(p)
    pt = np.zeros_like(p)
    vt = np.zeros_like(p)
    for i in range(N - 1, -1, -1):
        ci = c[:, :, None, :, i]
        v, vt = v * tl + p, vt * np.abs(tl) + pt
        p, pt = p * tl + ci, pt * np.abs(tl) + np.abs(ci)
    o = np.asarray(origin, dtype=np.float64).astype(LD)
    u = (p - o) / LD(h)
    d, G, inside = field_and_gradient(grid, u, h, outside)
    x = d - LD(inflation)
    pc, pdc = potential(x, epsilon)
    eta = LD(speed_epsilon)
    s = np.sqrt((v * v).sum(axis=-1) + eta * eta)
    wl = w.astype(LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        term = np.where(valid, wl * pc * s, LD(0))
        A = np.where(valid[..., None], (wl * pdc * s)[..., None] * G, LD(0))
        k2 = np.where(s == 0, LD(0), wl * pc / np.where(s == 0, LD(1), s))
        Bv = np.where(valid[..., None], k2[..., None] * v, LD(0))
    j = np.arange(N)
    pw = tl[..., None] ** j                                           # [B][K][Smax][1][N]: t^j
    dpw = np.where(j >= 1, j * tl[..., None] ** np.maximum(j - 1, 0), LD(0))
    gterm = A[..., None] * pw + Bv[..., None] * dpw                   # [B][K][Smax][3][N]
    agterm = np.abs(A)[..., None] * pw + np.abs(Bv)[..., None] * dpw
    cost, abs_cost = term.sum(axis=2), np.abs(term).sum(axis=2)
    grad, abs_grad = gterm.sum(axis=2), agterm.sum(axis=2)

    # ---- the a-priori bound (module docstring), float64 ----
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    gam, dmax = R.gammas(grid)
    gam = np.array(gam)
    du = EPS * ((2 * N + 4) * f64(pt) + 2 * np.abs(f64(p - o))) / h                  # [..][3]
    dv = EPS * (2 * N + 2) * f64(vt)
    inside3 = inside[..., None]
    dd = np.where(inside, (gam * du).sum(axis=-1) + EPS * 16 * dmax, 0.0)
    dG = np.where(inside3, (2 * gam * (du.sum(axis=-1, keepdims=True) - du) + EPS * (16 * dmax + 8 * gam)) / h, 0.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        xs, cs, dcs, ss, ws, vs, Gs = f64(x), f64(pc), np.abs(f64(pdc)), f64(s), np.abs(w), np.abs(f64(v)), np.abs(f64(G))
        dx = dd + EPS * np.abs(np.where(np.isfinite(xs), xs, 0.0))
        dc = dx + 4 * EPS * cs
        ddc = dx / epsilon + 3 * EPS * dcs
        ds = (dv * vs).sum(axis=-1) / ss + 4 * EPS * ss
        dterm = ws * (dc * ss + cs * ds) + 2 * EPS * np.abs(f64(term))
        dA = ws[..., None] * ((ddc * ss)[..., None] * Gs + (dcs * ds)[..., None] * Gs + (dcs * ss)[..., None] * dG) + 3 * EPS * np.abs(f64(A))
        dB = ws[..., None] * ((dc / ss)[..., None] * vs + (cs * dv.sum(axis=-1) / ss)[..., None]) + 3 * EPS * np.abs(f64(Bv))
    v3 = valid[..., None]
    dterm, dA, dB = np.where(valid, dterm, 0.0), np.where(v3, dA, 0.0), np.where(v3, dB, 0.0)
    pw64, dpw64 = f64(pw), f64(dpw)
    bt_cost = dterm.sum(axis=2)
    bt_grad = (dA[..., None] * pw64 + dB[..., None] * dpw64).sum(axis=2)
    Sf = S.astype(np.float64)
    bound_cost = bt_cost + EPS * (Sf + 6) * f64(abs_cost)
    bound_grad = bt_grad + EPS * (Sf[..., None, None] + 6 + 2 * j) * f64(abs_grad)

    # ---- fragile samples ----
    nz, ny, nx = grid.shape
    n = np.array([nx, ny, nz])
    uf = f64(u)
    gap = np.abs(uf - np.round(uf))
    jump = inside3 & (gap <= 2.0 * du)
    near = 1e-9 * np.maximum(1.0, np.abs(uf))
    edge = (np.abs(uf) <= near) | (np.abs(uf - (n - 1)) <= near)
    fragile = (jump | edge).any(axis=-1) & valid
    inside_valid = inside3 & v3
    out = dict(S=S, cost=cost, abs_cost=abs_cost, bound_cost=bound_cost, bound_terms_cost=bt_cost, grad=grad, abs_grad=abs_grad,
               bound_grad=bound_grad, bound_terms_grad=bt_grad, fragile=fragile,
               u_gap=float(np.where(inside_valid, gap, np.inf).min()), positive=int(((f64(pc) > 0) & valid).sum()),
               samples=int(valid.sum()))
    if want_terms:
        out.update(terms=f64(term), grad_terms=f64(gterm), w=w, t=t, valid=valid)
    return out


def butterfly(terms):
    """The rule's order of summation restated on float64 terms [..][Smax] (zeros beyond S add nothing): 64 partial sums, partial g
    over g, g + 64, .. in ascending order, joined by P[l] = P[l] + P[l xor off], off = 32 .. 1 -> [..]."""
    terms = np.asarray(terms, dtype=np.float64)
    smax = terms.shape[-1]
    P = np.zeros(terms.shape[:-1] + (64,))
    for first in range(0, smax, 64):
        chunk = terms[..., first:first + 64]
        P[..., :chunk.shape[-1]] = P[..., :chunk.shape[-1]] + chunk
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        P = P + P[..., lanes ^ off]
    assert (P == P[..., :1]).all() or np.isnan(P).any()
    return P[..., 0]
