"""Independent reference of the distance-field clearance check (include/mtg_hip.h, mtg_check_distance_field): numpy, longdouble,
vectorised over all samples of a batch.  The sample TIMES follow the float64 rule of the specification (they are part of it);
everything after them is longdouble: Horner positions, u by a true division, the lookup from the float32 voxels.

reference() returns every sample's clearance, a per-sample tolerance derived from the roundings of the float64 path

    tol = 2^-53 ( sum_a Gamma_a ((2 N + 4) ptilde_a + 2 |p_a - origin_a|) / h + 16 D_max )

(ptilde_a = sum_i |c_a,i| t^i: Horner's running error bound and the roundings of u; Gamma_a = largest |difference| of neighbouring
finite voxels along axis a: how far an error of u moves the value; D_max = largest finite |voxel|: the seven interpolation steps
and the subtraction of the inflation; nearest mode: 0, the value is a stored float) and which samples are FRAGILE: within
1e-9 max(1, |u_a|) of a domain edge (nearest: of a half-integer), or with a clearance within 2 tol + 1e-12 of zero -- the only
samples a comparison may leave out."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53


def sample_counts(times, dt):
    """S [B][K] by the rule itself: 2 + the number of i >= 1 with fl(i dt) < T (brute force over i)."""
    times = np.asarray(times, dtype=np.float64)
    S = np.full(times.shape, 2, dtype=np.int64)
    for idx in np.ndindex(times.shape):
        T = times[idx]
        if T > 0.0:
            i = np.arange(1, int(np.ceil(T / dt)) + 3, dtype=np.float64)
            S[idx] = 2 + int((i * dt < T).sum())
    return S


def sample_times(times, dt, S=None):
    """(t [B][K][Smax] float64, valid [B][K][Smax], S): t_i = fl(i dt), the last valid one T."""
    times = np.asarray(times, dtype=np.float64)
    S = sample_counts(times, dt) if S is None else S
    i = np.arange(int(S.max()))
    t = np.where(i == (S - 1)[..., None], times[..., None], i.astype(np.float64) * dt)
    return t, i < S[..., None], S


def spheres_field(lo, n, h, centres, radii):
    """float32 [nz][ny][nx]: distance to the nearest sphere's surface at the voxel centres lo + h (ix, iy, iz)."""
    ax = [lo[a] + h * np.arange(n[a]) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    d = np.full(z.shape, np.inf)
    for c, r in zip(centres, radii):
        d = np.minimum(d, np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r)
    return d.astype(np.float32)


def gammas(grid):
    """Gamma_x, Gamma_y, Gamma_z and D_max over the finite voxels."""
    g = grid.astype(np.float64)
    out = []
    for axis in (2, 1, 0):
        d = np.abs(np.diff(g, axis=axis))
        d = d[np.isfinite(d)]
        out.append(float(d.max()) if d.size else 0.0)
    fin = np.abs(g[np.isfinite(g)])
    return out, (float(fin.max()) if fin.size else 0.0)


def lookup(grid, u, outside, interpolation):
    """The field at voxel coordinates u [...][3] (longdouble) -> longdouble [...]."""
    nz, ny, nx = grid.shape
    n = np.array([nx, ny, nz])
    nan = np.isnan(u).any(axis=-1)
    u0 = np.where(np.isnan(u), 0, u)
    g = grid.astype(LD)
    if interpolation == "nearest":
        i = np.floor(u0 + LD(0.5))
        inside = ((i >= 0) & (i <= n - 1)).all(axis=-1)
        i = np.clip(i, 0, n - 1).astype(np.int64)
        d = g[i[..., 2], i[..., 1], i[..., 0]]
    else:
        inside = ((u0 >= 0) & (u0 <= n - 1)).all(axis=-1)
        i = np.clip(np.floor(u0), 0, n - 2).astype(np.int64)
        f = u0 - i
        d = np.zeros(u.shape[:-1], dtype=LD)
        with np.errstate(invalid="ignore"):
            for dz in (0, 1):
                for dy in (0, 1):
                    for dx in (0, 1):
                        w = ((f[..., 0] if dx else 1 - f[..., 0]) * (f[..., 1] if dy else 1 - f[..., 1])
                             * (f[..., 2] if dz else 1 - f[..., 2]))
                        v = g[i[..., 2] + dz, i[..., 1] + dy, i[..., 0] + dx]
                        d = d + w * v      # (finite voxels only: with others the result is whatever the specified arithmetic gives)
    d = np.where(inside, d, LD(outside))
    return np.where(nan, LD(np.nan), d)


def reference(coeffs, times, grid, origin, h, outside, interpolation, dt, inflation):
    """dict: S [B][K]; t, valid, clearance (longdouble), tol, fragile [B][K][Smax]; u [B][K][Smax][3]."""
    coeffs = np.asarray(coeffs, dtype=np.float64)
    t, valid, S = sample_times(times, dt)
    N = coeffs.shape[-1]
    c = coeffs[:, :, :3, :].astype(LD)                       # [B][K][3][N]
    tl = t.astype(LD)[:, :, :, None]                         # [B][K][Smax][1]
    p = np.zeros(t.shape + (3,), dtype=LD)
    pt = np.zeros(t.shape + (3,), dtype=LD)
    for i in range(N - 1, -1, -1):
        p = p * tl + c[:, :, None, :, i]
        pt = pt * np.abs(tl) + np.abs(c[:, :, None, :, i])
    o = np.asarray(origin, dtype=np.float64).astype(LD)
    u = (p - o) / LD(h)
    clearance = lookup(grid, u, outside, interpolation) - LD(inflation)
    nz, ny, nx = grid.shape
    n = np.array([nx, ny, nz])
    au = np.abs(u).astype(np.float64)
    near = 1e-9 * np.maximum(1.0, au)
    uf = u.astype(np.float64)
    if interpolation == "nearest":
        tol = np.zeros(t.shape)
        edge = (np.abs(uf + 0.5 - np.round(uf + 0.5)) <= near).any(axis=-1)
    else:
        gam, dmax = gammas(grid)
        tol = EPS * ((np.array(gam) * ((2 * N + 4) * pt + 2 * np.abs(p - o)).astype(np.float64)).sum(axis=-1) / h + 16.0 * dmax)
        edge = ((np.abs(uf) <= near) | (np.abs(uf - (n - 1)) <= near)).any(axis=-1)
    with np.errstate(invalid="ignore"):
        fragile = edge | (np.abs(clearance.astype(np.float64)) <= 2.0 * tol + 1e-12)
    return dict(S=S, t=t, valid=valid, clearance=np.where(valid, clearance, LD(np.inf)), tol=tol, fragile=fragile & valid, u=u)


def expected(ref):
    """Per-segment and per-trajectory answers of the reference (float64 / int): minimum, its first index, first failing sample,
    verdicts; a NaN fails and wins."""
    c = ref["clearance"].astype(np.float64)
    valid = ref["valid"]
    nan = np.isnan(c) & valid
    fails = ~(c > 0.0) & valid
    key = np.where(nan, -np.inf, c)                      # (a NaN wins the minimum, the first one its index)
    closest = key.argmin(axis=2)
    seg_min = np.where(nan.any(axis=2), np.nan, np.take_along_axis(c, closest[..., None], 2)[..., 0])
    first_failing = np.where(fails.any(axis=2), fails.argmax(axis=2), -1)
    seg_fail = fails.any(axis=2)
    fseg = np.where(seg_fail.any(axis=1), seg_fail.argmax(axis=1), -1)
    return dict(segment_clearance=seg_min, segment_closest_sample=closest, segment_first_failing_sample=first_failing,
                trajectory_feasible=(~seg_fail.any(axis=1)).astype(np.int32), first_failing_segment=fseg.astype(np.int32),
                segment_samples=ref["S"].astype(np.int32))
