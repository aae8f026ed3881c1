#!/usr/bin/env python3
"""Generates tests/golden/reference_obstacle_clearance_*.npz: sphere-obstacle clearances from the REFERENCE's own
Segment::computeMinMaxMagnitudeCandidates / selectMinMaxMagnitudeFromCandidates on trajectories its own solveLinear() produced.

Build container only (needs /root/reference).  Like make_reference_half_plane_golden.py, this script writes a C wrapper -- this
project's own text, below -- to a temporary directory, compiles there the six core sources of oracle/Makefile's REF_SRCS from the
reference tree where they lie, with -I oracle/ref_shim, runs the cases and commits ONLY DATA.  Nothing compiled from the
reference is kept, nothing is written under oracle/.

What is and is not the reference's code.  The reference has no obstacle check; what a caller of it writes is
Trajectory::offsetTrajectory(-centre) + computeMinMaxMagnitude(POSITION, {0, 1, 2}) per obstacle.  oc_check below does that per
(segment, obstacle) against the reference's public API:
    offset segment: the centre subtracted from the constant coefficient of dimensions 0-2   (what offsetTrajectory does)
    Segment::computeMinMaxMagnitudeCandidates(POSITION, 0, T, {0, 1, 2}, &candidates)       (the reference's, Jenkins-Traub below it)
    Segment::selectMinMaxMagnitudeFromCandidates(..., &minimum, &maximum)                  (the reference's)
    clearance = minimum.value - r - inflation
The loops over segments and obstacles, the verdict `clearance > 0` and the first-failure bookkeeping are this generator's lines.

Inputs.  The coefficients and times ALREADY COMMITTED for the six half-plane cases are read, not regenerated:
reference_feasibility_{n10_k2_d3, n10_k8_d3_fast, n12_k1_d4, n12_k4_d4}.npz and reference_half_plane_{n5_k3_d3, n7_k4_d4}.npz.

Obstacle sets, per case: `s16` -- numpy.random.default_rng(2024), 16 centres uniform in +-8 on each axis drawn first, then 16
radii uniform in [0.5, 1.5]; `s1` -- the first sphere of s16; `s16_inflated` -- s16 with inflation 0.3; for n10_k2_d3 also
`per_trajectory` -- default_rng(2025), 4 spheres per trajectory ([B][4][4], centres then radii, same ranges).

Per set s: `s/obstacles`, `s/inflation`, `s/clearance` [B][K][M] (every pair), `s/segment_feasible` [B][K] (bool),
`s/trajectory_feasible` [B], `s/first_failing_segment` [B] (-1: none), `s/first_failing_obstacle` [B] (-1: none),
`s/segment_clearance` [B][K], `s/segment_nearest_obstacle` [B][K], `s/robust` [B]; per case `max_position` [B]: the
reference's maximum of ||p|| over the trajectory's segments.  reference_obstacle_clearance_veneer_rows.txt: eight trajectories
of n10_k8_d3_fast with their s16 results as text, for the C++ veneer's test program.

robust (per trajectory): the reference's verdicts and first failures are unchanged with every radius changed by + and by -
1e-6 * max(1, scale), scale = r + inflation + ||c|| + max ||p|| -- the margin tests/helpers.py::assert_extrema_close gives the
reference's position minima (Jenkins-Traub scatters the multiple root at a resting end).  The cap on non-robust trajectories is
0 for every set here: asserted below and again by the tests.  If a set breaches it, change the seed, not the cap.

The files are written with fixed zip timestamps: a second run reproduces them bit for bit.

Run from the repository root:   python tests/golden/make_reference_obstacle_clearance_golden.py
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

WRAPPER = r"""
#include <mav_trajectory_generation/segment.h>

#include <cmath>
#include <vector>

namespace mtg = mav_trajectory_generation;

namespace {

// the segment with `centre` subtracted from the constant coefficient of dimensions 0-2 (centre == nullptr: as it is)
mtg::Segment make_segment(int n, int dim, const double* coeffs, double t, const double* centre) {
  mtg::Segment seg(n, dim);
  for (int d = 0; d < dim; ++d) {
    Eigen::VectorXd c(n);
    for (int j = 0; j < n; ++j) c[j] = coeffs[(size_t)d * n + j];
    if (centre && d < 3) c[0] -= centre[d];
    seg[d] = mtg::Polynomial(n, c);
  }
  seg.setTime(t);
  return seg;
}

bool min_max(const mtg::Segment& seg, mtg::Extremum* minimum, mtg::Extremum* maximum) {
  const std::vector<int> dims = {0, 1, 2};
  std::vector<mtg::Extremum> candidates;
  if (!seg.computeMinMaxMagnitudeCandidates(mtg::derivative_order::POSITION, 0.0, seg.getTime(), dims, &candidates)) return false;
  return seg.selectMinMaxMagnitudeFromCandidates(mtg::derivative_order::POSITION, 0.0, seg.getTime(), dims, candidates, minimum, maximum);
}

}  // namespace

extern "C" {

// One trajectory against m spheres (cx, cy, cz, r): clearance[k][m]; *max_position: maximum of ||p|| over the segments.
int oc_check(int n, int k, int dim, const double* coeffs, const double* times, const double* obstacles, int m, double inflation,
             double* clearance, double* max_position) {
  *max_position = 0.0;
  for (int s = 0; s < k; ++s) {
    mtg::Extremum minimum, maximum;
    if (!min_max(make_segment(n, dim, coeffs + (size_t)s * dim * n, times[s], nullptr), &minimum, &maximum)) return -1;
    if (maximum.value > *max_position) *max_position = maximum.value;
    for (int h = 0; h < m; ++h) {
      const double* o = obstacles + (size_t)h * 4;
      if (!min_max(make_segment(n, dim, coeffs + (size_t)s * dim * n, times[s], o), &minimum, &maximum)) return -1;
      clearance[(size_t)s * m + h] = minimum.value - o[3] - inflation;
    }
  }
  return 0;
}

}  // extern "C"
"""


def build_wrapper(tmp):
    wrap = os.path.join(tmp, "obstacle_clearance_wrap.cpp")
    with open(wrap, "w") as f:
        f.write(WRAPPER)
    core = os.path.join(REF, "mav_trajectory_generation")
    srcs = [os.path.join(core, "src", f) for f in ("polynomial.cpp", "vertex.cpp", "segment.cpp", "trajectory.cpp", "motion_defines.cpp",
                                                   "rpoly/rpoly_ak1.cpp")]
    lib = os.path.join(tmp, "libobstacle_clearance_ref.so")
    subprocess.check_call(["g++", "-O2", "-DNDEBUG", "-std=c++17", "-fPIC", "-w", "-shared", "-I" + os.path.join(ROOT, "oracle", "ref_shim"),
                           "-I" + os.path.join(core, "include"), "-o", lib, wrap] + srcs)
    so = ctypes.CDLL(lib)
    dp = ctypes.POINTER(ctypes.c_double)
    so.oc_check.argtypes = [ctypes.c_int] * 3 + [dp, dp, dp, ctypes.c_int, ctypes.c_double, dp, dp]
    return so


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def clearances(so, coeffs, times, obstacles, inflation):
    """[B][K][M] and max ||p|| [B]; obstacles [M][4] or [B][M][4]."""
    bsz, k, dim, n = coeffs.shape
    m = obstacles.shape[-2]
    out, pmax = np.zeros((bsz, k, m)), np.zeros((bsz,))
    one = ctypes.c_double(0.0)
    for b in range(bsz):
        obs = np.ascontiguousarray(obstacles[b] if obstacles.ndim == 3 else obstacles)
        row = np.zeros((k, m))
        assert so.oc_check(n, k, dim, _dp(np.ascontiguousarray(coeffs[b])), _dp(np.ascontiguousarray(times[b])), _dp(obs), m,
                           inflation, _dp(row), ctypes.byref(one)) == 0
        out[b], pmax[b] = row, one.value
    return out, pmax


def verdicts(clear):
    """From [B][K][M] clearances: segment_feasible, trajectory_feasible, first failing segment / obstacle, per-segment minimum and
    the obstacle that attains it (the first on a tie)."""
    fails = ~(clear > 0.0)
    seg_fail = fails.any(axis=2)
    traj = (~seg_fail.any(axis=1)).astype(np.int32)
    fseg = np.where(seg_fail.any(axis=1), seg_fail.argmax(axis=1), -1).astype(np.int32)
    fobs = np.array([-1 if s < 0 else int(fails[b, s].argmax()) for b, s in enumerate(fseg)], dtype=np.int32)
    return ~seg_fail, traj, fseg, fobs, clear.min(axis=2), clear.argmin(axis=2).astype(np.int32)


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


def s16():
    rng = np.random.default_rng(2024)
    centres = rng.uniform(-8.0, 8.0, (16, 3))
    radii = rng.uniform(0.5, 1.5, 16)
    return np.concatenate([centres, radii[:, None]], axis=1)


def per_trajectory(bsz):
    rng = np.random.default_rng(2025)
    centres = rng.uniform(-8.0, 8.0, (bsz, 4, 3))
    radii = rng.uniform(0.5, 1.5, (bsz, 4))
    return np.concatenate([centres, radii[..., None]], axis=2)


def write_veneer_rows(path, coeffs, times, out, n_each=4):
    """Text rows for tests/cpp/test_obstacle_clearance_veneer.cpp: the first n_each feasible and n_each infeasible trajectories
    under s16, with the reference's verdict, first failing segment and obstacle and minimum clearance."""
    feas = out["s16/trajectory_feasible"]
    pick = sorted(list(np.flatnonzero(feas == 1)[:n_each]) + list(np.flatnonzero(feas == 0)[:n_each]))
    _, k, dim, n = coeffs.shape
    obs = out["s16/obstacles"]
    with open(path, "w") as f:
        f.write("# N K D rows M inflation / M x (cx cy cz r) / per row: times, coefficients [K][D][N], then verdict, first failing "
                "segment, first failing obstacle, minimum clearance, scale\n")
        f.write(f"{n} {k} {dim} {len(pick)} {obs.shape[0]} 0.0\n")
        for o in obs:
            f.write(" ".join(repr(float(v)) for v in o) + "\n")
        for b in pick:
            f.write(" ".join(repr(float(v)) for v in times[b]) + "\n")
            for s in range(k):
                for d in range(dim):
                    f.write(" ".join(repr(float(v)) for v in coeffs[b, s, d]) + "\n")
            scale = float((obs[:, 3] + np.sqrt((obs[:, :3] ** 2).sum(axis=1))).max() + out["max_position"][b])
            f.write(f"{int(feas[b])} {int(out['s16/first_failing_segment'][b])} {int(out['s16/first_failing_obstacle'][b])} "
                    f"{float(out['s16/segment_clearance'][b].min())!r} {scale!r}\n")


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
            sets = [("s16", s16(), 0.0), ("s1", s16()[:1], 0.0), ("s16_inflated", s16(), 0.3)]
            if name == "n10_k2_d3":
                sets.append(("per_trajectory", per_trajectory(bsz), 0.0))
            out = {"obstacle_sets": np.array([s[0] for s in sets])}
            for sname, obs, inflation in sets:
                clear, pmax = clearances(so, coeffs, times, obs, inflation)
                seg, traj, fseg, fobs, seg_c, seg_o = verdicts(clear)
                scale = obs[..., 3] + inflation + np.sqrt((obs[..., :3] ** 2).sum(axis=-1)) + (pmax[:, None] if obs.ndim == 3 else pmax.max())
                delta = MARGIN * np.maximum(1.0, scale)
                if obs.ndim == 2:   # a shared set: the margin of the trajectory with the largest ||p|| serves all (the wider one)
                    delta = np.broadcast_to(delta, obs.shape[:-1])
                robust = np.ones((bsz,), dtype=bool)
                for sign in (-1.0, 1.0):
                    moved = obs.copy()
                    moved[..., 3] += sign * delta
                    seg_s, _, fseg_s, fobs_s, _, _ = verdicts(clearances(so, coeffs, times, moved, inflation)[0])
                    robust &= (seg_s == seg).all(axis=1) & (fseg_s == fseg) & (fobs_s == fobs)
                n_bad = int((~robust).sum())
                assert n_bad == 0, (name, sname, n_bad)
                out["max_position"] = pmax
                for key, value in (("obstacles", obs), ("inflation", np.float64(inflation)), ("clearance", clear), ("segment_feasible", seg),
                                   ("trajectory_feasible", traj), ("first_failing_segment", fseg), ("first_failing_obstacle", fobs),
                                   ("segment_clearance", seg_c), ("segment_nearest_obstacle", seg_o), ("robust", robust)):
                    out[f"{sname}/{key}"] = value
                print(f"{name}/{sname}: feasible {int(traj.sum())}/{bsz}, failing not in segment 0: {int((fseg > 0).sum())}, "
                      f"smallest |clearance| {np.abs(clear).min():.2e}, non-robust {n_bad}")
            if name == "n10_k8_d3_fast":
                write_veneer_rows(os.path.join(HERE, "reference_obstacle_clearance_veneer_rows.txt"), coeffs, times, out)
            path = os.path.join(HERE, f"reference_obstacle_clearance_{name}.npz")
            save_deterministic(path, out)
            size = os.path.getsize(path)
            print(f"  wrote {path} ({size} B)")
            assert size <= 500 * 1000, size


if __name__ == "__main__":
    sys.exit(main())
