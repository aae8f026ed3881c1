#!/usr/bin/env python3
"""Generates tests/golden/reference_keep_out_*.npz: keep-out zone clearances from the REFERENCE's own candidate searches and
evaluation on trajectories its own solveLinear() produced.

Build container only (needs /root/reference).  Like make_reference_obstacle_clearance_golden.py, this script writes a C wrapper --
this project's own text, below -- to a temporary directory, compiles there the six core sources of oracle/Makefile's REF_SRCS
from the reference tree where they lie, with -I oracle/ref_shim, runs the cases and commits ONLY DATA.  Nothing compiled from the
reference is kept, nothing is written under oracle/.

What is and is not the reference's code.  The reference has no keep-out check; ko_check below builds one per (segment, zone) on
the reference's public API:
    q_j = sum_dim n_jd p_dim as a Polynomial; Polynomial::computeMinMaxCandidates(0, T, 0, &c)    (0, T and the real roots of q_j',
                                                                                                  Jenkins-Traub below it)
    d_ij = (offset_i - offset_j) + (n_j - n_i) . p as a Polynomial; Polynomial::getRoots(0, &r)     (Jenkins-Traub) and
    Polynomial::selectMinMaxCandidatesFromRoots(0, T, r, &c)                                       (the reference's filter)
    p(t) per axis by Polynomial::evaluate(t, 0); clearance = min over the candidates of max_j (offset_j - n_j . p(t)) - inflation
The loops over segments, zones and planes, the envelope's max, the verdict `clearance > 0` and the first-failure bookkeeping
are this generator's lines.

Inputs.  The coefficients and times ALREADY COMMITTED for the six half-plane cases are read, not regenerated:
reference_feasibility_{n10_k2_d3, n10_k8_d3_fast, n12_k1_d4, n12_k4_d4}.npz and reference_half_plane_{n5_k3_d3, n7_k4_d4}.npz.

Zone sets, per case: `z16` -- numpy.random.default_rng(SEED_SHARED), 16 box centres uniform in +-8 on each axis drawn first, then
16 x 3 sizes uniform in [0.5, 2.5], the even boxes axis-aligned (HalfPlane::createBoundingBox's planes, order and signs), the
odd ones rotated by a seeded orthogonal matrix (drawn after the sizes, one 3 x 3 normal matrix per odd box, QR); `z1` -- the
first box of z16; `z16_inflated` -- z16 with inflation 0.3; for n10_k2_d3 also `per_trajectory` -- default_rng(SEED_PER), 4
boxes per trajectory ([B][4][6][4], same ranges, all rotated).

Per set s: `s/zones`, `s/inflation`, `s/clearance` [B][K][M] (every pair), `s/segment_feasible` [B][K] (bool),
`s/trajectory_feasible` [B], `s/first_failing_segment` [B] (-1: none), `s/first_failing_zone` [B] (-1: none),
`s/segment_clearance` [B][K], `s/segment_nearest_zone` [B][K], `s/robust` [B]; per case `max_position` [B]: the reference's
maximum of ||p|| over the trajectory's segments.  reference_keep_out_veneer_rows.txt: eight trajectories of n10_k8_d3_fast with
their z16 results as text, for the C++ veneer's test program.

robust (per trajectory): the reference's verdicts and first failures are unchanged with every offset moved by + and by -
1e-6 * max(1, scale), scale = max_j |offset_j| + inflation + max ||p||.  The cap on non-robust trajectories is 0 for every set
here: asserted below and again by the tests.  If a set breaches it, change the seed, not the cap.

The files are written with fixed zip timestamps: a second run reproduces them bit for bit.

Run from the repository root:   python tests/golden/make_reference_keep_out_golden.py
"""
import ctypes
import io
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
MARGIN = 1e-6
SEED_SHARED, SEED_PER = 2026, 2027

WRAPPER = r"""
#include <mav_trajectory_generation/polynomial.h>
#include <mav_trajectory_generation/segment.h>

#include <cmath>
#include <vector>

namespace mtg = mav_trajectory_generation;

namespace {

mtg::Polynomial projected(int n, const double* coeffs, const double* v, double constant) {
  Eigen::VectorXd c(n);
  for (int j = 0; j < n; ++j) c[j] = v[0] * coeffs[j] + v[1] * coeffs[n + j] + v[2] * coeffs[2 * n + j];
  c[0] += constant;
  return mtg::Polynomial(n, c);
}

double max_norm(int n, int dim, const double* coeffs, double t) {
  mtg::Segment seg(n, dim);
  for (int d = 0; d < dim; ++d) {
    Eigen::VectorXd c(n);
    for (int j = 0; j < n; ++j) c[j] = coeffs[(size_t)d * n + j];
    seg[d] = mtg::Polynomial(n, c);
  }
  seg.setTime(t);
  const std::vector<int> dims = {0, 1, 2};
  std::vector<mtg::Extremum> candidates;
  mtg::Extremum minimum, maximum;
  if (!seg.computeMinMaxMagnitudeCandidates(mtg::derivative_order::POSITION, 0.0, t, dims, &candidates)) return NAN;
  if (!seg.selectMinMaxMagnitudeFromCandidates(mtg::derivative_order::POSITION, 0.0, t, dims, candidates, &minimum, &maximum)) return NAN;
  return maximum.value;
}

}  // namespace

extern "C" {

// One trajectory against m zones of p planes (nx, ny, nz, offset): clearance[k][m]; *max_position: maximum of ||p|| over the segments.
int ko_check(int n, int k, int dim, const double* coeffs, const double* times, const double* zones, int m, int p, double inflation,
             double* clearance, double* max_position) {
  *max_position = 0.0;
  for (int s = 0; s < k; ++s) {
    const double* c = coeffs + (size_t)s * dim * n;
    const double T = times[s];
    const double reach = max_norm(n, dim, c, T);
    if (!(reach == reach)) return -1;
    if (reach > *max_position) *max_position = reach;
    mtg::Polynomial axis[3] = {mtg::Polynomial(n), mtg::Polynomial(n), mtg::Polynomial(n)};
    for (int d = 0; d < 3; ++d) {
      Eigen::VectorXd v(n);
      for (int j = 0; j < n; ++j) v[j] = c[(size_t)d * n + j];
      axis[d] = mtg::Polynomial(n, v);
    }
    for (int h = 0; h < m; ++h) {
      const double* z = zones + (size_t)h * 4 * p;
      std::vector<double> all, found;
      for (int j = 0; j < p; ++j) {
        if (!projected(n, c, z + 4 * j, 0.0).computeMinMaxCandidates(0.0, T, 0, &found)) return -1;
        all.insert(all.end(), found.begin(), found.end());
      }
      for (int i = 0; i < p; ++i)
        for (int j = i + 1; j < p; ++j) {
          const double v[3] = {z[4 * j] - z[4 * i], z[4 * j + 1] - z[4 * i + 1], z[4 * j + 2] - z[4 * i + 2]};
          Eigen::VectorXcd roots;
          if (!projected(n, c, v, z[4 * i + 3] - z[4 * j + 3]).getRoots(0, &roots)) continue;   // (a constant: no crossing)
          if (!mtg::Polynomial::selectMinMaxCandidatesFromRoots(0.0, T, roots, &found)) return -1;
          all.insert(all.end(), found.begin(), found.end());
        }
      double best = INFINITY;
      for (double t : all) {
        const double x[3] = {axis[0].evaluate(t, 0), axis[1].evaluate(t, 0), axis[2].evaluate(t, 0)};
        double top = -INFINITY;
        for (int j = 0; j < p; ++j) {
          const double hj = z[4 * j + 3] - (z[4 * j] * x[0] + z[4 * j + 1] * x[1] + z[4 * j + 2] * x[2]);
          if (hj > top) top = hj;
        }
        if (top - inflation < best) best = top - inflation;
      }
      clearance[(size_t)s * m + h] = best;
    }
  }
  return 0;
}

}  // extern "C"
"""


def build_wrapper(tmp):
    wrap = os.path.join(tmp, "keep_out_wrap.cpp")
    with open(wrap, "w") as f:
        f.write(WRAPPER)
    core = os.path.join(REF, "mav_trajectory_generation")
    srcs = [os.path.join(core, "src", f) for f in ("polynomial.cpp", "vertex.cpp", "segment.cpp", "trajectory.cpp", "motion_defines.cpp",
                                                   "rpoly/rpoly_ak1.cpp")]
    lib = os.path.join(tmp, "libkeep_out_ref.so")
    subprocess.check_call(["g++", "-O2", "-DNDEBUG", "-std=c++17", "-fPIC", "-w", "-shared", "-I" + os.path.join(ROOT, "oracle", "ref_shim"),
                           "-I" + os.path.join(core, "include"), "-o", lib, wrap] + srcs)
    so = ctypes.CDLL(lib)
    dp = ctypes.POINTER(ctypes.c_double)
    so.ko_check.argtypes = [ctypes.c_int] * 3 + [dp, dp, dp, ctypes.c_int, ctypes.c_int, ctypes.c_double, dp, dp]
    return so


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def clearances(so, coeffs, times, zones, inflation):
    """[B][K][M] and max ||p|| [B]; zones [M][P][4] or [B][M][P][4]."""
    bsz, k, dim, n = coeffs.shape
    m, p = zones.shape[-3], zones.shape[-2]
    out, pmax = np.zeros((bsz, k, m)), np.zeros((bsz,))
    one = ctypes.c_double(0.0)
    for b in range(bsz):
        z = np.ascontiguousarray(zones[b] if zones.ndim == 4 else zones)
        row = np.zeros((k, m))
        assert so.ko_check(n, k, dim, _dp(np.ascontiguousarray(coeffs[b])), _dp(np.ascontiguousarray(times[b])), _dp(z), m, p,
                           inflation, _dp(row), ctypes.byref(one)) == 0
        out[b], pmax[b] = row, one.value
    return out, pmax


def verdicts(clear):
    """From [B][K][M] clearances: segment_feasible, trajectory_feasible, first failing segment / zone, per-segment minimum and the
    zone that attains it (the first on a tie)."""
    fails = ~(clear > 0.0)
    seg_fail = fails.any(axis=2)
    traj = (~seg_fail.any(axis=1)).astype(np.int32)
    fseg = np.where(seg_fail.any(axis=1), seg_fail.argmax(axis=1), -1).astype(np.int32)
    fzone = np.array([-1 if s < 0 else int(fails[b, s].argmax()) for b, s in enumerate(fseg)], dtype=np.int32)
    return ~seg_fail, traj, fseg, fzone, clear.min(axis=2), clear.argmin(axis=2).astype(np.int32)


def save_deterministic(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same data gives the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, value in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o600 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def box(centre, size, rotation=None):
    """[6][4]: per axis the minimum face with +r, then the maximum face with -r (rotation None: the coordinate axes)."""
    r = np.eye(3) if rotation is None else rotation
    out = np.zeros((6, 4))
    for axis in range(3):
        e = r[:, axis]
        out[2 * axis, :3], out[2 * axis, 3] = e, np.dot(centre - size[axis] / 2.0 * e, e)
        out[2 * axis + 1, :3], out[2 * axis + 1, 3] = -e, -np.dot(centre + size[axis] / 2.0 * e, e)
    return out


def z16():
    """(zones [16][6][4], centres, sizes)."""
    rng = np.random.default_rng(SEED_SHARED)
    centres = rng.uniform(-8.0, 8.0, (16, 3))
    sizes = rng.uniform(0.5, 2.5, (16, 3))
    zones = np.zeros((16, 6, 4))
    for m in range(16):
        zones[m] = box(centres[m], sizes[m], np.linalg.qr(rng.standard_normal((3, 3)))[0] if m % 2 else None)
    return zones, centres, sizes


def per_trajectory(bsz):
    rng = np.random.default_rng(SEED_PER)
    centres = rng.uniform(-8.0, 8.0, (bsz, 4, 3))
    sizes = rng.uniform(0.5, 2.5, (bsz, 4, 3))
    zones = np.zeros((bsz, 4, 6, 4))
    for b in range(bsz):
        for m in range(4):
            zones[b, m] = box(centres[b, m], sizes[b, m], np.linalg.qr(rng.standard_normal((3, 3)))[0])
    return zones


def write_veneer_rows(path, coeffs, times, out, n_each=4):
    """Text rows for tests/cpp/test_keep_out_veneer.cpp: the first n_each feasible and n_each infeasible trajectories under z16,
    with the reference's verdict, first failing segment and zone and minimum clearance."""
    feas = out["z16/trajectory_feasible"]
    pick = sorted(list(np.flatnonzero(feas == 1)[:n_each]) + list(np.flatnonzero(feas == 0)[:n_each]))
    assert len(pick) == 2 * n_each
    _, k, dim, n = coeffs.shape
    zones = out["z16/zones"]
    with open(path, "w") as f:
        f.write("# N K D rows M P inflation / M x P x (nx ny nz offset) / per row: times, coefficients [K][D][N], then verdict, first "
                "failing segment, first failing zone, minimum clearance, scale\n")
        f.write(f"{n} {k} {dim} {len(pick)} {zones.shape[0]} {zones.shape[1]} 0.0\n")
        for plane in zones.reshape(-1, 4):
            f.write(" ".join(repr(float(v)) for v in plane) + "\n")
        for b in pick:
            f.write(" ".join(repr(float(v)) for v in times[b]) + "\n")
            for s in range(k):
                for d in range(dim):
                    f.write(" ".join(repr(float(v)) for v in coeffs[b, s, d]) + "\n")
            scale = float(np.abs(zones[..., 3]).max() + out["max_position"][b])
            f.write(f"{int(feas[b])} {int(out['z16/first_failing_segment'][b])} {int(out['z16/first_failing_zone'][b])} "
                    f"{float(out['z16/segment_clearance'][b].min())!r} {scale!r}\n")


CASES = [("n10_k2_d3", "reference_feasibility_n10_k2_d3.npz"), ("n10_k8_d3_fast", "reference_feasibility_n10_k8_d3_fast.npz"),
         ("n12_k1_d4", "reference_feasibility_n12_k1_d4.npz"), ("n12_k4_d4", "reference_feasibility_n12_k4_d4.npz"),
         ("n5_k3_d3", "reference_half_plane_n5_k3_d3.npz"), ("n7_k4_d4", "reference_half_plane_n7_k4_d4.npz")]


def main():
    assert os.path.exists(os.path.join(REF, "mav_trajectory_generation", "src", "polynomial.cpp")), "needs /root/reference"
    with tempfile.TemporaryDirectory() as tmp:
        so = build_wrapper(tmp)
        for name, source in CASES:
            z = np.load(os.path.join(HERE, source))
            coeffs, times = z["coeffs"], z["times"]
            bsz = coeffs.shape[0]
            sets = [("z16", z16()[0], 0.0), ("z1", z16()[0][:1], 0.0), ("z16_inflated", z16()[0], 0.3)]
            if name == "n10_k2_d3":
                sets.append(("per_trajectory", per_trajectory(bsz), 0.0))
            out = {"zone_sets": np.array([s[0] for s in sets])}
            for sname, zones, inflation in sets:
                clear, pmax = clearances(so, coeffs, times, zones, inflation)
                seg, traj, fseg, fzone, seg_c, seg_z = verdicts(clear)
                reach = np.abs(zones[..., 3]).max(axis=-1)                          # [M] or [B][M]
                scale = reach + inflation + (pmax[:, None] if zones.ndim == 4 else pmax.max())
                delta = MARGIN * np.maximum(1.0, scale)
                robust = np.ones((bsz,), dtype=bool)
                for sign in (-1.0, 1.0):
                    moved = zones.copy()
                    moved[..., 3] += sign * delta[..., None]
                    seg_s, _, fseg_s, fzone_s, _, _ = verdicts(clearances(so, coeffs, times, moved, inflation)[0])
                    robust &= (seg_s == seg).all(axis=1) & (fseg_s == fseg) & (fzone_s == fzone)
                n_bad = int((~robust).sum())
                assert n_bad == 0, (name, sname, n_bad)
                out["max_position"] = pmax
                for key, value in (("zones", zones), ("inflation", np.float64(inflation)), ("clearance", clear), ("segment_feasible", seg),
                                   ("trajectory_feasible", traj), ("first_failing_segment", fseg), ("first_failing_zone", fzone),
                                   ("segment_clearance", seg_c), ("segment_nearest_zone", seg_z), ("robust", robust)):
                    out[f"{sname}/{key}"] = value
                print(f"{name}/{sname}: feasible {int(traj.sum())}/{bsz}, failing not in segment 0: {int((fseg > 0).sum())}, "
                      f"smallest |clearance| {np.abs(clear).min():.2e}, non-robust {n_bad}")
            if name == "n10_k8_d3_fast":
                write_veneer_rows(os.path.join(HERE, "reference_keep_out_veneer_rows.txt"), coeffs, times, out)
            path = os.path.join(HERE, f"reference_keep_out_{name}.npz")
            save_deterministic(path, out)
            size = os.path.getsize(path)
            print(f"  wrote {path} ({size} B)")
            assert size <= 500 * 1000, size


if __name__ == "__main__":
    sys.exit(main())
