"""Independent replay of the certified distance-field check (include/mtg_hip.h, mtg_certify_distance_field): numpy, longdouble,
vectorised over all nodes of a level of a whole batch.  It follows the same tree -- the node TIMES m = fl((2 j + 1) w) and
w = T 2^-(d+1) are float64, they are part of the rule -- but has its own arithmetic after them: positions by a longdouble
Horner, the Taylor coefficients q_k = sum_j C(j, k) c_j m^(j-k) from the binomial formula (not the shift), u by a true
division, the lookup of tests/distance_field_ref.py.

Per decision it knows the margin by which it was taken, and per value a tolerance derived from the roundings of the float64
path (EPS = 2^-53, N the coefficient count, h the voxel size):

    tol_c    the sampled check's bound (distance_field_ref): EPS (sum_a Gamma_a ((2 N + 4) ptilde_a + 2 |p_a - o_a|) / h + 16 D_max)
    tol_R_a  EPS ((2 N + 4) sum_j |c_a,j| (|m| + w)^j + 4 Rh_a): the shift's running error summed over the orders (the binomial
             theorem collects sum_k w^k sum_j C(j, k) |c_j| |m|^(j-k) into (|m| + w)^j), and the four roundings of Rh_a
    tol_b    tol_c + L ||tol_R|| + 8 EPS (|Dc| + inflation + L Rh): the value at the clamped point, the reach, the bound's own sums

A segment is FRAGILE, and only then left out of an exact comparison, if one of its decisions is that close to flipping: a sample's
c or a node's bound within 2 tol + 1e-12 of zero, a voxel coordinate or a face of the node's box within 1e-9 max(1, |u|, rho) of
a face of the grid, or a second, different c within 2 tol_c of the segment's lowest one (the closest time is then not unique)."""
import math

import numpy as np

import distance_field_ref as R

LD = np.longdouble
EPS = 2.0 ** -53
S_SLACK = LD(2.0) ** -36
COLLIDES, FREE, UNDECIDED_DEPTH, UNDECIDED_BUDGET = 0, 1, 2, 3


def _evaluate(c, m, w, grid, origin, h, outside, lipschitz, inflation, gam, dmax):
    """Nodes n: c [n][3][N] longdouble coefficients, m, w [n] float64 -> dict of [n] arrays."""
    N = c.shape[-1]
    ml, wl, am = m.astype(LD), w.astype(LD), np.abs(m).astype(LD)
    o = np.asarray(origin, dtype=np.float64).astype(LD)
    p = np.zeros(c.shape[:2], dtype=LD)
    pt = np.zeros(c.shape[:2], dtype=LD)
    wide = np.zeros(c.shape[:2], dtype=LD)
    for i in range(N - 1, -1, -1):
        p = p * ml[:, None] + c[:, :, i]
        pt = pt * am[:, None] + np.abs(c[:, :, i])
        wide = wide * (am + wl)[:, None] + np.abs(c[:, :, i])
    reach = np.zeros(c.shape[:2], dtype=LD)
    for k in range(1, N):
        q = np.zeros(c.shape[:2], dtype=LD)
        for j in range(k, N):
            q = q + LD(math.comb(j, k)) * c[:, :, j] * ml[:, None] ** (j - k)
        reach = reach + np.abs(q) * wl[:, None] ** k
    A = pt + np.abs(o)
    rh_a = reach * (1 + S_SLACK) + S_SLACK * A
    rh = np.sqrt((rh_a * rh_a).sum(axis=1)) * (1 + S_SLACK)
    u = (p - o) / LD(h)
    nz, ny, nx = grid.shape
    top = np.array([nx, ny, nz], dtype=np.float64) - 1.0
    cl = R.lookup(grid, u, outside, "trilinear") - LD(inflation)
    rho = rh_a / LD(h) * (1 + S_SLACK)
    with np.errstate(invalid="ignore"):
        inside = ((u - rho >= 0) & (u + rho <= top)).all(axis=1)
        touches = ((u + rho >= 0) & (u - rho <= top)).all(axis=1)
        uc = np.where(np.isnan(u), u, np.clip(u, 0, top))
        dc = R.lookup(grid, uc, outside, "trilinear")
        b_in = dc - LD(inflation) - LD(lipschitz) * rh - S_SLACK * (np.abs(dc) + LD(inflation) + 2 * LD(lipschitz) * LD(h))
        b_in = np.where(touches, b_in, LD(np.inf))
        b_out = np.where(inside, LD(np.inf), LD(outside) - LD(inflation))
        bound = np.where(np.isnan(b_in) | np.isnan(b_out), LD(np.nan), np.minimum(b_in, b_out))
        bound = np.where((np.isnan(u - rho) | np.isnan(u + rho)).any(axis=1), LD(np.nan), bound)
    # tolerances and margins (float64 is enough for them)
    f = lambda x: np.asarray(x, dtype=np.float64)
    g = np.array(gam)
    tol_c = EPS * ((g * f((2 * N + 4) * pt + 2 * np.abs(p - o))).sum(axis=1) / h + 16.0 * dmax)
    tol_r = EPS * ((2 * N + 4) * f(wide + np.abs(o)) + 4.0 * f(rh_a))
    with np.errstate(invalid="ignore"):
        tol_b = tol_c + lipschitz * np.sqrt((tol_r * tol_r).sum(axis=1)) + 8.0 * EPS * f(np.abs(dc) + LD(inflation) + LD(lipschitz) * rh)
        uf, rf = f(u), f(rho)
        near = 1e-9 * np.maximum(1.0, np.maximum(np.abs(uf), rf))
        faces = [uf, uf - top, uf - rf, uf + rf - top, uf + rf, uf - rf - top]
        edge = np.zeros(len(m), dtype=bool)
        for d in faces:
            edge |= (np.abs(d) <= near).any(axis=1)
        fragile = edge | (np.abs(f(cl)) <= 2.0 * tol_c + 1e-12) | (np.abs(f(bound)) <= 2.0 * tol_b + 1e-12)
    return dict(c=cl, bound=bound, tol_c=tol_c, tol_b=np.where(np.isfinite(tol_b), tol_b, 0.0), fragile=fragile, rh=rh)


def replay(coeffs, times, grid, origin, h, outside, lipschitz, inflation, min_depth=4, max_depth=16, max_frontier=1024):
    """dict of [B][K] arrays: result, nodes, depth, lower_bound, sampled, closest_time, first_failing_time (float64 / int), the two
    tolerances tol_lower and tol_sampled, fragile, and largest_frontier."""
    coeffs = np.asarray(coeffs, dtype=np.float64)
    times = np.asarray(times, dtype=np.float64)
    B, K = times.shape
    S = B * K
    c_all = coeffs[:, :, :3, :].reshape(S, 3, -1).astype(LD)
    T = times.reshape(S)
    gam, dmax = R.gammas(grid)
    with np.errstate(invalid="ignore"):
        lone = ~(T > 0.0)
    fails = np.zeros(S, bool)
    undecided = np.zeros(S, bool)
    budget = np.zeros(S, bool)
    fragile = np.zeros(S, bool)
    nodes = np.zeros(S, np.int64)
    depth = np.zeros(S, np.int64)
    lower = np.full(S, np.inf, dtype=LD)
    lower_nan = np.zeros(S, bool)
    tol_lower = np.zeros(S)
    tol_sampled = np.zeros(S)
    largest = np.zeros(S, np.int64)
    fail_time = np.full(S, np.inf)
    rec_seg, rec_m, rec_c, rec_tol = [], [], [], []

    def level(seg, j, d, last):
        w = np.where(lone[seg], 0.0, T[seg] * 2.0 ** -(d + 1))
        m = np.where(lone[seg], np.where(np.isnan(T[seg]), T[seg], 0.0), (2.0 * j + 1.0) * w)
        e = _evaluate(c_all[seg], m, w, grid, origin, h, outside, lipschitz, inflation, gam, dmax)
        cf, bf = e["c"].astype(np.float64), e["bound"].astype(np.float64)
        with np.errstate(invalid="ignore"):
            fl = ~(cf > 0.0)
            cert = ~fl & (bf > 0.0)
        terminal = fl | cert | last
        np.logical_or.at(fails, seg[fl], True)
        np.logical_or.at(undecided, seg[terminal & ~fl & ~cert], True)
        np.logical_or.at(fragile, seg[e["fragile"]], True)
        np.minimum.at(fail_time, seg[fl], np.where(np.isnan(m[fl]), -np.inf, m[fl]))
        np.add.at(nodes, seg, 1)
        np.maximum.at(depth, seg, d)
        tb = e["bound"][terminal]
        np.logical_or.at(lower_nan, seg[terminal][np.isnan(tb)], True)
        np.minimum.at(lower, seg[terminal][~np.isnan(tb)], tb[~np.isnan(tb)])
        np.maximum.at(tol_lower, seg[terminal], e["tol_b"][terminal])
        np.maximum.at(tol_sampled, seg, e["tol_c"])
        rec_seg.append(seg), rec_m.append(m), rec_c.append(e["c"]), rec_tol.append(e["tol_c"])
        return ~terminal

    lone_ids = np.nonzero(lone)[0]
    if lone_ids.size:
        level(lone_ids, np.zeros(lone_ids.size, np.int64), 0, True)
        depth[lone_ids] = 0
    ids = np.nonzero(~lone)[0]
    seg = np.repeat(ids, 1 << min_depth)
    j = np.tile(np.arange(1 << min_depth, dtype=np.int64), ids.size)
    d = min_depth
    while seg.size:
        np.maximum.at(largest, seg, np.bincount(seg, minlength=S)[seg])
        alive = level(seg, j, d, d == max_depth)
        survivors = np.bincount(seg[alive], minlength=S)
        over = 2 * survivors > max_frontier
        budget |= over
        keep = alive & ~over[seg]
        seg, j = np.repeat(seg[keep], 2), (2 * np.repeat(j[keep], 2) + np.tile([0, 1], int(keep.sum())))
        d += 1
    # the lowest sample and its time: ties exact in float64 go to the smaller m; a different value within 2 tol is fragile
    rs, rm = np.concatenate(rec_seg), np.concatenate(rec_m)
    rc, rt = np.concatenate(rec_c), np.concatenate(rec_tol)
    sampled = np.full(S, np.nan)
    closest = np.full(S, np.nan)
    key = np.where(np.isnan(rc), LD(-np.inf), rc)
    order = np.lexsort((rm, key.astype(np.float64), rs))
    rs, rm, rc, rt, key = rs[order], rm[order], rc[order], rt[order], key[order]
    first = np.r_[True, rs[1:] != rs[:-1]]
    start = np.nonzero(first)[0]
    sampled[rs[start]] = rc[start].astype(np.float64)
    closest[rs[start]] = rm[start]
    lowest = np.repeat(key[start], np.diff(np.r_[start, rs.size]))
    with np.errstate(invalid="ignore"):
        close = (key.astype(np.float64) != lowest.astype(np.float64)) & (np.abs((key - lowest).astype(np.float64)) <= 2.0 * rt)
    np.logical_or.at(fragile, rs[close], True)
    result = np.where(fails, COLLIDES, np.where(budget, UNDECIDED_BUDGET, np.where(undecided, UNDECIDED_DEPTH, FREE)))
    lower_f = np.where(lower_nan, np.nan, lower.astype(np.float64))
    lower_f = np.where(budget, -np.inf, lower_f)
    shape = lambda a: a.reshape(B, K)
    return dict(result=shape(result), nodes=shape(nodes), depth=shape(depth), lower_bound=shape(lower_f), sampled=shape(sampled),
                closest_time=shape(closest), first_failing_time=shape(np.where(fails, np.where(fail_time == -np.inf, np.nan, fail_time), np.nan)),
                tol_lower=shape(tol_lower), tol_sampled=shape(tol_sampled), fragile=shape(fragile), largest_frontier=shape(largest))
