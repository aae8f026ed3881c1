#!/usr/bin/env python3
"""Generates tests/golden/reference_recursive_feasibility_*.npz: verdicts, whole-segment bounds and section counts of the
reference's recursive input-feasibility test (FeasibilityRecursive, mav_trajectory_generation_ros/src/feasibility_recursive.cpp)
on trajectories its own solveLinear() produced.

Build container only (needs /root/reference).  Like make_reference_half_plane_golden.py (whose stand-in headers, include list and
deterministic npz writer are imported from it), this script writes a C wrapper -- this project's own text, below -- to a temporary
directory, compiles there the six core sources of oracle/Makefile's REF_SRCS from the reference tree where they lie, with
-I oracle/ref_shim, runs the cases and commits ONLY DATA.  Nothing compiled from the reference is kept, nothing is written under
oracle/.

What is and is not the reference's code.  feasibility_recursive.cpp is tried first (reference_unit_compiles below).  Recorded
outcome: it does NOT compile against the unchanged Eigen stand-in of oracle/ref_shim -- six errors, all from the three head<3>()
calls (lines 162, 164, 301), a member template the stand-in's matrix class lacks and that cannot be supplied from outside the
class.  So the recursion in the wrapper (rz_section, rz_recurse, rz_segment) is this generator's own lines, a restatement of
FeasibilityRecursive::checkInputFeasibility / recursiveFeasibility against the reference's public API.  The reference's, with
Jenkins-Traub below them:
    Polynomial::getRoots(derivative, &roots)                           all complex roots of one axis' derivative polynomial
    Polynomial::selectMinMaxFromRoots(t1, t2, derivative, roots, ..)   extrema over {t1, t2, real roots inside [t1, t2]}
    Polynomial::computeMinMax(0, T, derivative, ..)                    the yaw checks
    Segment::evaluate(t, derivative)                                   thrust and velocity at a section's ends
The generator's: the norm over the first three components (sqrt of x^2 + y^2 + z^2 summed in that order), adding gravity
(0, 0, 9.81) to the acceleration, the order of the tests inside a section and the depth-first recursion with the first half
first (both restated from the reference's lines 133-297), the loop over the segments, the section counter, and the reporting
of the whole-segment bounds.  Unlike the reference's function, rz_section does not return at the first failing test: it computes
every bound whose limit is set and then applies the tests in the reference's order, which gives the result of the
early-returning form by construction and yields the bounds for `segment_bounds` whatever the verdict.

Inputs.  The coefficients and times ALREADY COMMITTED in reference_feasibility_{n10_k8_d3_slow, n10_k8_d3_thrust,
n10_k8_d3_fast, n10_k2_d3, n12_k1_d4, n12_k4_d4}.npz and reference_half_plane_n7_k4_d4.npz (the odd-N zero padding) are read,
not regenerated, and not stored again: a golden file names its `source`.

Limit sets: the ones named in the source files with their min_section_time_s; plus `velocity` (v_max = 7) for n10_k8_d3_fast,
`loose` (f_min 2, f_max 25, v_max 6, omega_xy_max 3: no trajectory fails) for n10_k8_d3_slow, and for n7_k4_d4, whose source
has none, `defaults` (the reference's six default limits: these fast trajectories all fail on thrust) and `wide` (f_max 220,
v_max 100, omega_z_max 70, omega_z_dot_max 150, at the scale of these polynomials, whose dropped highest power makes them wild:
a mix).

Per set s: `s/limits` [6] (NaN = absent; f_min, f_max, v_max, omega_xy_max, omega_z_max, omega_z_dot_max),
`s/min_section_time_s`, `s/segment_result` [B][K], `s/trajectory_result` [B], `s/first_failing_segment` [B] (-1: none),
`s/segment_bounds` [B][K][6] (f_lower_bound, f_upper_bound, v_upper_bound and roll/pitch bound of the section [0, T]; |yaw rate|
max, |yaw acceleration| max; each for EVERY quantity whose limit is set -- the thrust bounds when any of f_min, f_max,
omega_xy_max is -- whatever the verdict; NaN otherwise), `s/segment_sections` [B][K] (calls of the recursion that got past the
minimum-section-time test) and `s/robust` [B].  reference_recursive_feasibility_veneer_rows.txt: eight trajectories of
n12_k4_d4 / all_six as text, for the C++ veneer's test program.

robust, exactly as in make_reference_feasibility_golden.py: a trajectory is robust under a limit set if (i) the per-segment
verdicts are unchanged with every limit scaled by 1 - 1e-6 and by 1 + 1e-6, and (ii) no real root in [0, T] of the (up to nine)
polynomials the set needs lies within 1e-8 T of an INTERIOR split point T j / 2^d, 0 < j < 2^d,
d <= ceil(log2(T / min_section_time_s)).  At most 1 % of the trajectories of any (case, limit set), and never more than
max(1, B // 100), may be non-robust: asserted here and again by the tests.  If a set breaches the cap, change the set, not the
cap.

The files are written with fixed zip timestamps: a second run reproduces them bit for bit.

Run from the repository root:   python tests/golden/make_reference_recursive_feasibility_golden.py
"""
import ctypes
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_half_plane_golden as hp   # noqa: E402  (stand-in headers, include list, deterministic writer)

ROOT, REF = hp.ROOT, hp.REF
NAN = float("nan")
G = 9.81
ROOT_CAP = 32   # root times stored per segment for the robustness test: 9 + 8 + 7 at N = 12, three axes each -> at most 72

WRAPPER = r"""
#include <mav_trajectory_generation/polynomial.h>
#include <mav_trajectory_generation/segment.h>
#include <mav_trajectory_generation/motion_defines.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <utility>
#include <vector>

namespace mtg = mav_trajectory_generation;

namespace {

const double kGravity = 9.81;   // mav_msgs::kGravity upstream; gravity_ = (0, 0, kGravity)

struct Limits {
  double v[6];   // f_min, f_max, v_max, omega_xy_max, omega_z_max, omega_z_dot_max; NaN: absent
  double min_section;
  bool has(int i) const { return v[i] == v[i]; }
};

struct Roots {
  std::vector<Eigen::VectorXcd> acc, jerk, snap;   // per axis, empty if the limits do not need them
};

struct Bounds {
  double f_lower, f_upper, v_upper, omega_xy;
};

mtg::Segment make_segment(int n, int dim, const double* coeffs, double t) {
  mtg::Segment seg(n, dim);
  for (int d = 0; d < dim; ++d) {
    Eigen::VectorXd c(n);
    for (int j = 0; j < n; ++j) c[j] = coeffs[(size_t)d * n + j];
    seg[d] = mtg::Polynomial(n, c);
  }
  seg.setTime(t);
  return seg;
}

double norm3(const mtg::Segment& seg, double t, int derivative, double gz) {
  const Eigen::VectorXd v = seg.evaluate(t, derivative);
  const double x = v[0], y = v[1], z = v[2] + gz;
  return std::sqrt(x * x + y * y + z * z);
}

double sq(double x) { return x * x; }

// One section [t1, t2]: every bound whose limit is set, then the reference's tests in the reference's order.
// Returns a result code, or -1: some bound exceeds its limit without proving a violation (split).
int rz_section(const mtg::Segment& seg, const Roots& roots, const Limits& lim, double t1, double t2, Bounds* out) {
  const bool thrust_limits = lim.has(0) || lim.has(1), any_thrust = thrust_limits || lim.has(3);
  int early = 0;   // the first failing test among the ones the reference returns from before the bounds are complete
  if (thrust_limits) {
    const double f1 = norm3(seg, t1, mtg::derivative_order::ACCELERATION, kGravity);
    const double f2 = norm3(seg, t2, mtg::derivative_order::ACCELERATION, kGravity);
    if (lim.has(0) && std::min(f1, f2) < lim.v[0]) early = 3;
    else if (lim.has(1) && std::max(f1, f2) > lim.v[1]) early = 2;
  }
  double v_sqr = 0.0, f_min_sqr = 0.0, f_max_sqr = 0.0, j_sqr = 0.0;
  if (lim.has(2)) {
    const double v1 = norm3(seg, t1, mtg::derivative_order::VELOCITY, 0.0);
    const double v2 = norm3(seg, t2, mtg::derivative_order::VELOCITY, 0.0);
    if (!early && std::max(v1, v2) > lim.v[2]) early = 4;
    for (int i = 0; i < 3; ++i) {
      std::pair<double, double> lo, hi;
      seg[i].selectMinMaxFromRoots(t1, t2, mtg::derivative_order::VELOCITY, roots.acc[i], &lo, &hi);
      if (!early && std::max(sq(lo.second), sq(hi.second)) > sq(lim.v[2])) early = 4;
      v_sqr += sq(std::max(std::abs(lo.second), std::abs(hi.second)));
    }
  }
  if (any_thrust) {
    for (int i = 0; i < 3; ++i) {
      std::pair<double, double> lo, hi;
      seg[i].selectMinMaxFromRoots(t1, t2, mtg::derivative_order::ACCELERATION, roots.jerk[i], &lo, &hi);
      const double g = i == 2 ? kGravity : 0.0;
      const double f_lo = lo.second + g, f_hi = hi.second + g;
      const double big = std::max(std::abs(f_lo), std::abs(f_hi));
      if (!early && lim.has(1) && big > lim.v[1]) early = 2;
      if (!(f_lo * f_hi < 0.0)) f_min_sqr += sq(std::min(std::abs(f_lo), std::abs(f_hi)));
      f_max_sqr += sq(big);
    }
  }
  if (lim.has(3)) {
    for (int i = 0; i < 3; ++i) {
      std::pair<double, double> lo, hi;
      seg[i].selectMinMaxFromRoots(t1, t2, mtg::derivative_order::JERK, roots.snap[i], &lo, &hi);
      j_sqr += sq(std::max(std::abs(lo.second), std::abs(hi.second)));
    }
  }
  out->f_lower = std::sqrt(f_min_sqr);
  out->f_upper = std::sqrt(f_max_sqr);
  out->v_upper = std::sqrt(v_sqr);
  out->omega_xy = f_min_sqr > 1.0e-6 ? std::sqrt(j_sqr / f_min_sqr) : std::numeric_limits<double>::max();
  if (early) return early;
  if (lim.has(0) && out->f_upper < lim.v[0]) return 3;
  if (lim.has(1) && out->f_lower > lim.v[1]) return 2;
  if ((lim.has(0) && out->f_lower < lim.v[0]) || (lim.has(1) && out->f_upper > lim.v[1]) || (lim.has(2) && out->v_upper > lim.v[2]) ||
      (lim.has(3) && out->omega_xy > lim.v[3]))
    return -1;
  return 0;
}

int rz_recurse(const mtg::Segment& seg, const Roots& roots, const Limits& lim, double t1, double t2, int depth, int* sections,
               int* max_depth) {
  if (t2 - t1 < lim.min_section) return 1;
  ++*sections;
  *max_depth = std::max(*max_depth, depth);
  Bounds b;
  const int r = rz_section(seg, roots, lim, t1, t2, &b);
  if (r >= 0) return r;
  const double t_half = (t1 + t2) / 2;
  const int first = rz_recurse(seg, roots, lim, t1, t_half, depth + 1, sections, max_depth);
  if (first != 0) return first;
  return rz_recurse(seg, roots, lim, t_half, t2, depth + 1, sections, max_depth);
}

// One segment: verdict; bounds[6]; sections; root_times[cap] (real roots in [0, T] of the polynomials the limits need, NaN-padded)
int rz_segment(const mtg::Segment& seg, const Limits& lim, double* bounds, int* sections, int* max_depth, double* root_times, int cap) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int q = 0; q < 6; ++q) bounds[q] = nan;
  for (int q = 0; q < cap; ++q) root_times[q] = nan;
  *sections = 0;
  if (!(seg.D() == 3 || seg.D() == 4)) return 1;
  const double T = seg.getTime();
  Roots roots;
  int n_roots = 0;
  auto find = [&](std::vector<Eigen::VectorXcd>* set, int derivative) {
    set->resize(3);
    for (int i = 0; i < 3; ++i) {
      seg[i].getRoots(derivative, &(*set)[i]);
      std::vector<double> cand;
      mtg::Polynomial::selectMinMaxCandidatesFromRoots(0.0, T, (*set)[i], &cand);
      for (size_t c = 2; c < cand.size() && n_roots < cap; ++c) root_times[n_roots++] = cand[c];   // (0 and 1 are the ends)
    }
  };
  const bool any_thrust = lim.has(0) || lim.has(1) || lim.has(3);
  if (lim.has(2)) find(&roots.acc, mtg::derivative_order::ACCELERATION);
  if (any_thrust) find(&roots.jerk, mtg::derivative_order::JERK);
  if (lim.has(3)) find(&roots.snap, mtg::derivative_order::SNAP);
  Bounds top;
  rz_section(seg, roots, lim, 0.0, T, &top);
  if (any_thrust) { bounds[0] = top.f_lower; bounds[1] = top.f_upper; }
  if (lim.has(2)) bounds[2] = top.v_upper;
  if (lim.has(3)) bounds[3] = top.omega_xy;
  int result = rz_recurse(seg, roots, lim, 0.0, T, 0, sections, max_depth);
  if (seg.D() == 4) {
    std::pair<double, double> lo, hi;
    if (lim.has(4)) {
      seg[3].computeMinMax(0.0, T, mtg::derivative_order::ANGULAR_VELOCITY, &lo, &hi);
      bounds[4] = std::max(std::abs(lo.second), std::abs(hi.second));
      if (result == 0 && bounds[4] > lim.v[4]) result = 6;
    }
    if (lim.has(5)) {
      seg[3].computeMinMax(0.0, T, mtg::derivative_order::ANGULAR_ACCELERATION, &lo, &hi);
      bounds[5] = std::max(std::abs(lo.second), std::abs(hi.second));
      if (result == 0 && bounds[5] > lim.v[5]) result = 7;
    }
  }
  return result;
}

}  // namespace

extern "C" {

// One trajectory: segment_result [K], segment_bounds [K][6], segment_sections [K], root_times [K][cap]; returns the trajectory
// verdict (the first segment in segment order that is not feasible), *first = that segment or -1
int rz_check(int n, int k, int dim, const double* coeffs, const double* times, const double* limits, double min_section,
             int* segment_result, int* first, double* segment_bounds, int* segment_sections, int* max_depth, double* root_times,
             int cap) {
  Limits lim;
  for (int i = 0; i < 6; ++i) lim.v[i] = std::abs(limits[i]);
  lim.min_section = std::abs(min_section);
  int result = 0;
  *first = -1;
  for (int s = 0; s < k; ++s) {
    const mtg::Segment seg = make_segment(n, dim, coeffs + (size_t)s * dim * n, times[s]);
    segment_result[s] = rz_segment(seg, lim, segment_bounds + (size_t)s * 6, segment_sections + s, max_depth,
                                   root_times + (size_t)s * cap, cap);
    if (segment_result[s] != 0 && *first < 0) { *first = s; result = segment_result[s]; }
  }
  return result;
}

}  // extern "C"
"""


def reference_unit_compiles(tmp):
    """feasibility_recursive.cpp itself against oracle/ref_shim and the stand-in headers: does it compile?"""
    src = os.path.join(REF, "mav_trajectory_generation_ros", "src", "feasibility_recursive.cpp")
    r = subprocess.run(["g++", "-O0", "-std=c++17", "-fPIC", "-w", "-fsyntax-only"] + hp._includes(tmp) + [src], capture_output=True, text=True)
    return r.returncode == 0, r.stderr


def build_wrapper(tmp):
    wrap = os.path.join(tmp, "recursive_wrap.cpp")
    with open(wrap, "w") as f:
        f.write(WRAPPER)
    core = os.path.join(REF, "mav_trajectory_generation")
    srcs = [os.path.join(core, "src", f) for f in ("polynomial.cpp", "vertex.cpp", "segment.cpp", "trajectory.cpp", "motion_defines.cpp",
                                                   "rpoly/rpoly_ak1.cpp")]
    lib = os.path.join(tmp, "librecursive_ref.so")
    subprocess.check_call(["g++", "-O2", "-DNDEBUG", "-std=c++17", "-fPIC", "-w", "-shared"] + hp._includes(tmp) + ["-o", lib, wrap] + srcs)
    so = ctypes.CDLL(lib)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    so.rz_check.argtypes = [ctypes.c_int] * 3 + [dp, dp, dp, ctypes.c_double, ip, ip, dp, ip, ip, dp, ctypes.c_int]
    return so


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def limits_of(**kw):
    names = ("f_min", "f_max", "v_max", "omega_xy_max", "omega_z_max", "omega_z_dot_max")
    assert set(kw) <= set(names)
    return np.array([abs(kw[n]) if n in kw else NAN for n in names])


DEFAULTS = dict(f_min=0.5 * G, f_max=1.5 * G, v_max=3.0, omega_xy_max=math.pi / 2, omega_z_max=math.pi / 2, omega_z_dot_max=2 * math.pi)

# name, source of (coeffs, times) and of its named limit sets, further [(limit set name, limits, min_section_time_s)]
CASES = [
    ("n10_k8_d3_slow", "reference_feasibility_n10_k8_d3_slow.npz", [("loose", limits_of(f_min=2.0, f_max=25.0, v_max=6.0, omega_xy_max=3.0), 0.05)]),
    ("n10_k8_d3_thrust", "reference_feasibility_n10_k8_d3_thrust.npz", []),
    ("n10_k8_d3_fast", "reference_feasibility_n10_k8_d3_fast.npz", [("velocity", limits_of(v_max=7.0), 0.05)]),
    ("n10_k2_d3", "reference_feasibility_n10_k2_d3.npz", []),
    ("n12_k1_d4", "reference_feasibility_n12_k1_d4.npz", []),
    ("n12_k4_d4", "reference_feasibility_n12_k4_d4.npz", []),
    ("n7_k4_d4", "reference_half_plane_n7_k4_d4.npz", [
        ("defaults", limits_of(**DEFAULTS), 0.05),
        ("wide", limits_of(f_max=220.0, v_max=100.0, omega_z_max=70.0, omega_z_dot_max=150.0), 0.05)]),
]
VENEER_ROWS = ("n12_k4_d4", "all_six", 8)


def check_batch(so, coeffs, times, limits, min_section):
    bsz, k, dim, n = coeffs.shape
    seg = np.zeros((bsz, k), dtype=np.int32)
    sections = np.zeros((bsz, k), dtype=np.int32)
    bounds = np.zeros((bsz, k, 6))
    roots = np.zeros((bsz, k, 3 * ROOT_CAP))
    traj = np.zeros((bsz,), dtype=np.int32)
    first = np.zeros((bsz,), dtype=np.int32)
    f, depth = ctypes.c_int(0), ctypes.c_int(0)
    lim = np.ascontiguousarray(limits, dtype=np.float64)
    for b in range(bsz):
        row, rows = np.zeros((k,), dtype=np.int32), np.zeros((k,), dtype=np.int32)
        traj[b] = so.rz_check(n, k, dim, _dp(np.ascontiguousarray(coeffs[b])), _dp(np.ascontiguousarray(times[b])), _dp(lim), min_section,
                              _ip(row), ctypes.byref(f), _dp(bounds[b]), _ip(rows), ctypes.byref(depth), _dp(roots[b]), 3 * ROOT_CAP)
        seg[b], sections[b], first[b] = row, rows, f.value
    return seg, traj, first, bounds, sections, roots, depth.value


def split_margin(root_times, T, min_section):
    """min over the root times of the distance to the nearest INTERIOR split point, in units of T."""
    if not T > min_section:
        return np.inf
    depth = max(0, int(math.ceil(math.log2(T / min_section))))
    if depth == 0:
        return np.inf
    m = 2 ** depth
    t = root_times[np.isfinite(root_times)]
    x = t / T * m
    j = np.clip(np.rint(x), 1, m - 1)
    return float(np.min(np.abs(x - j)) / m) if t.size else np.inf


def write_veneer_rows(path, coeffs, times, limits, min_section, seg, traj, first, robust, n_rows):
    """Text rows for tests/cpp/test_recursive_feasibility_veneer.cpp: robust trajectories, one of every verdict first."""
    pick = []
    for code in np.unique(traj):
        pick.append(int(np.flatnonzero((traj == code) & robust)[0]))
    for b in np.flatnonzero(robust):
        if len(pick) >= n_rows:
            break
        if int(b) not in pick:
            pick.append(int(b))
    pick = sorted(pick[:n_rows])
    _, k, dim, n = coeffs.shape
    with open(path, "w") as f:
        f.write("# N K D rows / limits (f_min f_max v_max omega_xy_max omega_z_max omega_z_dot_max; nan: absent) min_section_time_s / "
                "per row: times, coefficients [K][D][N], segment verdicts, trajectory verdict, first failing segment\n")
        f.write(f"{n} {k} {dim} {len(pick)}\n")
        f.write(" ".join(repr(float(v)) for v in list(limits) + [min_section]) + "\n")
        for b in pick:
            f.write(" ".join(repr(float(v)) for v in times[b]) + "\n")
            for s in range(k):
                for d in range(dim):
                    f.write(" ".join(repr(float(v)) for v in coeffs[b, s, d]) + "\n")
            f.write(" ".join(str(int(v)) for v in seg[b]) + "\n")
            f.write(f"{int(traj[b])} {int(first[b])}\n")


def main():
    assert os.path.exists(os.path.join(REF, "mav_trajectory_generation", "src", "polynomial.cpp")), "needs /root/reference"
    seen, later = {}, {}
    deepest, most_sections = 0, 0
    with tempfile.TemporaryDirectory() as tmp:
        hp._write_stand_ins(tmp)
        ok, err = reference_unit_compiles(tmp)
        errors = [l for l in err.splitlines() if "error" in l]
        print("feasibility_recursive.cpp against oracle/ref_shim:", "COMPILES -- use it instead of the wrapper's own recursion" if ok else
              f"does not compile ({len(errors)} errors, first: {errors[0].strip()[:150] if errors else '?'}); the recursion is the generator's")
        so = build_wrapper(tmp)
        for name, source, extra_sets in CASES:
            z = np.load(os.path.join(HERE, source))
            coeffs, times = z["coeffs"], z["times"]
            bsz, k, dim, n = coeffs.shape
            sets = [(str(s), z[f"{s}/limits"], float(z[f"{s}/min_section_time_s"])) for s in (z["limit_sets"] if "limit_sets" in z.files else [])]
            sets += extra_sets
            out = {"source": np.array(source), "limit_sets": np.array([s[0] for s in sets])}
            for sname, limits, min_section in sets:
                seg, traj, first, bounds, sections, roots, depth = check_batch(so, coeffs, times, limits, min_section)
                robust = np.ones((bsz,), dtype=bool)
                for scale in (1.0 - 1e-6, 1.0 + 1e-6):
                    seg_s = check_batch(so, coeffs, times, limits * scale, min_section)[0]
                    robust &= (seg_s == seg).all(axis=1)
                n_scale = int((~robust).sum())
                for b in range(bsz):
                    for s in range(k):
                        if split_margin(roots[b, s], times[b, s], min_section) < 1e-8:
                            robust[b] = False
                n_bad = int((~robust).sum())
                assert n_bad <= 0.01 * bsz and n_bad <= max(1, bsz // 100), (name, sname, n_bad)
                assert 5 not in seg
                assert np.isfinite(roots[..., -1]).sum() == 0   # the root table was large enough
                out[f"{sname}/limits"], out[f"{sname}/min_section_time_s"] = limits, np.float64(min_section)
                out[f"{sname}/segment_result"], out[f"{sname}/trajectory_result"], out[f"{sname}/first_failing_segment"] = seg, traj, first
                out[f"{sname}/segment_bounds"], out[f"{sname}/segment_sections"], out[f"{sname}/robust"] = bounds, sections, robust
                mix = {int(c): int((traj == c).sum()) for c in np.unique(traj)}
                for c, cnt in mix.items():
                    seen[c] = seen.get(c, 0) + cnt
                    later[c] = later.get(c, 0) + int(((traj == c) & (first > 0)).sum())
                deepest, most_sections = max(deepest, depth), max(most_sections, int(sections.sum(axis=1).max()))
                print(f"{name}/{sname}: verdicts {mix}, verdict changes under scaled limits {n_scale}, non-robust {n_bad}, "
                      f"most sections per trajectory {int(sections.sum(axis=1).max())}")
                if (name, sname) == VENEER_ROWS[:2]:
                    write_veneer_rows(os.path.join(HERE, "reference_recursive_feasibility_veneer_rows.txt"), coeffs, times, limits, min_section,
                                      seg, traj, first, robust, VENEER_ROWS[2])
            path = os.path.join(HERE, f"reference_recursive_feasibility_{name}.npz")
            hp.save_deterministic(path, out)
            size = os.path.getsize(path)
            print(f"  wrote {path} ({size} B)")
            assert size <= 300 * 1000, size
    print("trajectory verdicts over the set:", seen, "with a failing segment that is not the first:", later, "deepest section:", deepest,
          "most sections in a trajectory:", most_sections)
    for code in (0, 1, 2, 3, 4, 6, 7):
        assert seen.get(code, 0) >= 5, code
        if code != 0:
            assert later.get(code, 0) >= 1, code
    assert 5 not in seen


if __name__ == "__main__":
    sys.exit(main())
