#!/usr/bin/env python3
"""Generates tests/golden/reference_feasibility_*.npz: verdicts of the REFERENCE's own FeasibilityAnalytic
(mav_trajectory_generation_ros/src/feasibility_analytic.cpp) on trajectories its own solveLinear() produced.

Build container only (needs /root/reference).  This script writes stand-in headers and a C wrapper -- all of them this project's
own text, below -- to a temporary directory, compiles there
    mav_trajectory_generation_ros/src/{feasibility_analytic,input_constraints}.cpp  and the six core sources of oracle/Makefile's
    REF_SRCS
from the reference tree where they lie, with -I oracle/ref_shim (the Eigen / glog container stand-ins every other anchor here
uses), runs the cases and commits ONLY DATA: coefficients, times, limit sets, verdicts and bounds.  Nothing compiled from the
reference is kept, nothing is written under oracle/.

What is and is not the reference's code: FeasibilityAnalytic::checkInputFeasibility(const Segment&) and everything below it
(thrust segment, candidate searches, Jenkins-Traub roots, the roll/pitch recursion), InputConstraints, createRandomVertices,
estimateSegmentTimes and solveLinear are the reference's.  feasibility_base.cpp cannot be compiled against the Eigen stand-in
(head<3>(), cross, normalize, finished() are missing), so the wrapper supplies the two FeasibilityBase constructors (they only
set gravity_ = (0, 0, kGravity)) and the first-failing-segment loop of checkInputFeasibilityTrajectory: those ten lines are not
the reference's.  Stand-in headers: ros/ros.h (empty ROS_*_STREAM macros), mav_msgs/default_values.h (kGravity = 9.81, its
upstream value), Eigen/StdVector (Eigen/Core + an empty EIGEN_MAKE_ALIGNED_OPERATOR_NEW), yaml-cpp/yaml.h (a do-nothing
YAML::Node).

Per case: `coeffs` [B][K][D][N] exactly as solveLinear() left them (the tests feed these bits, not a re-solve), `times` [B][K];
per limit set s: `s/limits` [6] (NaN = absent; f_min, f_max, v_max, omega_xy_max, omega_z_max, omega_z_dot_max),
`s/min_section_time_s`, `s/segment_result` [B][K], `s/trajectory_result` [B], `s/first_failing_segment` [B] (-1: none),
`s/segment_bounds` [B][K][6] (thrust min, thrust max, velocity max, roll/pitch bound of the whole segment, |yaw rate| max,
|yaw acceleration| max -- through the reference's public Segment / Polynomial API, for EVERY quantity whose limit is set, whether
or not an earlier check failed; NaN otherwise) and `s/robust` [B].

robust: a verdict is compared only where the reference's own answer does not hang on the last digits.  A trajectory is robust
under a limit set if (i) the reference returns the same per-segment verdicts with every limit scaled by 1 - 1e-6 and by
1 + 1e-6, and (ii) when omega_xy_max is set, no thrust or jerk candidate time (public computeMinMaxMagnitudeCandidateTimes) lies
within 1e-8 T of an INTERIOR split point T j / 2^d, 0 < j < 2^d, d <= ceil(log2(T / min_section_time_s)).  0 and T are not split
points (the end itself is a candidate with the same value).  At most 1 % of the trajectories of any (case, limit set), and never
more than max(1, B // 100), may be non-robust: asserted here and again by the tests.  If a case breaches the cap, change its
seed range, not the cap.

Run from the repository root:   python tests/golden/make_reference_feasibility_golden.py
"""
import ctypes
import math
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
NAN = float("nan")
G = 9.81

STAND_INS = {
    "ros/ros.h": """#pragma once
#define ROS_ERROR_STREAM(x) do { } while (0)
#define ROS_WARN_STREAM(x) do { } while (0)
#define ROS_INFO_STREAM(x) do { } while (0)
#define ROS_DEBUG_STREAM(x) do { } while (0)
""",
    "mav_msgs/default_values.h": """#pragma once
namespace mav_msgs { const double kGravity = 9.81; }
""",
    "Eigen/StdVector": """#pragma once
#include <Eigen/Core>
#ifndef EIGEN_MAKE_ALIGNED_OPERATOR_NEW
#define EIGEN_MAKE_ALIGNED_OPERATOR_NEW
#endif
""",
    "yaml-cpp/yaml.h": """#pragma once
#include <string>
namespace YAML {
struct Node {
  Node operator[](const std::string&) const { return Node(); }
  template <class T> Node& operator=(const T&) { return *this; }
  template <class T> T as() const { return T(); }
  explicit operator bool() const { return false; }
};
}
""",
}

WRAPPER = r"""
#include <mav_trajectory_generation/polynomial_optimization_linear.h>
#include <mav_trajectory_generation/trajectory.h>
#include <mav_trajectory_generation/vertex.h>
#include <mav_trajectory_generation_ros/feasibility_analytic.h>
#include <mav_msgs/default_values.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

namespace mtg = mav_trajectory_generation;

// ---- NOT the reference's: feasibility_base.cpp does not compile against the Eigen stand-in ------------------------------
namespace mav_trajectory_generation {
FeasibilityBase::FeasibilityBase() { gravity_[0] = 0.0; gravity_[1] = 0.0; gravity_[2] = mav_msgs::kGravity; }
FeasibilityBase::FeasibilityBase(const InputConstraints& c) : input_constraints_(c) {
  gravity_[0] = 0.0; gravity_[1] = 0.0; gravity_[2] = mav_msgs::kGravity;
}
}
// --------------------------------------------------------------------------------------------------------------------------

namespace {

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

template <int N>
int make_one(int k, int dim, double box, double v, double a, unsigned long long seed, double* coeffs, double* times) {
  const mtg::Vertex::Vector vertices = mtg::createRandomVertices(mtg::derivative_order::SNAP, k, Eigen::VectorXd::Constant(dim, -box),
                                                                 Eigen::VectorXd::Constant(dim, box), seed);
  const std::vector<double> segment_times = mtg::estimateSegmentTimes(vertices, v, a);
  mtg::PolynomialOptimization<N> opt(dim);
  opt.setupFromVertices(vertices, segment_times, mtg::derivative_order::SNAP);
  opt.solveLinear();
  mtg::Segment::Vector segments;
  opt.getSegments(&segments);
  for (int s = 0; s < k; ++s) {
    times[s] = segments[s].getTime();
    for (int d = 0; d < dim; ++d) {
      const Eigen::VectorXd c = segments[s][d].getCoefficients(0);
      for (int j = 0; j < N; ++j) coeffs[((size_t)s * dim + d) * N + j] = c[j];
    }
  }
  return 0;
}

mtg::FeasibilityAnalytic make_checker(const double* limits, double min_section) {
  mtg::InputConstraints ic;
  for (int i = 0; i < 6; ++i)
    if (limits[i] == limits[i]) ic.addConstraint(i, limits[i]);
  mtg::FeasibilityAnalytic::Settings settings;
  settings.setMinSectionTimeS(min_section);
  return mtg::FeasibilityAnalytic(settings, ic);
}

const std::vector<int> kXYZ = {0, 1, 2};

mtg::Segment thrust_segment_of(const mtg::Segment& seg) {   // f = acceleration + g, through public calls
  const int n = seg.N() - 2;
  mtg::Segment thrust(n, 3);
  thrust.setTime(seg.getTime());
  for (int d = 0; d < 3; ++d) {
    Eigen::VectorXd acc = seg[d].getCoefficients(mtg::derivative_order::ACCELERATION);
    Eigen::VectorXd c(n);
    for (int j = 0; j < n; ++j) c[j] = acc[j];
    if (d == 2) c[0] += mav_msgs::kGravity;
    thrust[d] = mtg::Polynomial(n, c);
  }
  return thrust;
}

}  // namespace

extern "C" {

int fz_make(int n, int k, int dim, double box, double v, double a, unsigned long long seed, double* coeffs, double* times) {
  switch (n) {
    case 10: return make_one<10>(k, dim, box, v, a, seed, coeffs, times);
    case 12: return make_one<12>(k, dim, box, v, a, seed, coeffs, times);
    default: return -1;
  }
}

// verdicts of one trajectory: segment_result [K]; returns the trajectory verdict, *first = first failing segment or -1
int fz_check(int n, int k, int dim, const double* coeffs, const double* times, const double* limits, double min_section,
             int* segment_result, int* first) {
  const mtg::FeasibilityAnalytic checker = make_checker(limits, min_section);
  int result = 0;
  *first = -1;
  for (int s = 0; s < k; ++s) {
    const mtg::Segment seg = make_segment(n, dim, coeffs + (size_t)s * dim * n, times[s]);
    segment_result[s] = (int)checker.checkInputFeasibility(seg);
    if (segment_result[s] != 0 && *first < 0) { *first = s; result = segment_result[s]; }   // (the loop of feasibility_base.cpp:97-107)
  }
  return result;
}

// bounds [K][6] through the public API; cand_times [K][2][cap] thrust / jerk candidate times, NaN-padded
void fz_bounds(int n, int k, int dim, const double* coeffs, const double* times, const double* limits, double* bounds,
               double* cand_times, int cap) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  auto set = [&](int i) { return limits[i] == limits[i]; };
  for (int s = 0; s < k; ++s) {
    const mtg::Segment seg = make_segment(n, dim, coeffs + (size_t)s * dim * n, times[s]);
    const double T = seg.getTime();
    double* b = bounds + (size_t)s * 6;
    for (int q = 0; q < 6; ++q) b[q] = nan;
    for (int q = 0; q < 2 * cap; ++q) cand_times[(size_t)s * 2 * cap + q] = nan;
    if (!(dim == 3 || dim == 4)) continue;
    double f_min = nan;
    if (set(0) || set(1) || set(3)) {
      const mtg::Segment thrust = thrust_segment_of(seg);
      std::vector<mtg::Extremum> cand;
      thrust.computeMinMaxMagnitudeCandidates(0, 0.0, T, kXYZ, &cand);
      b[0] = std::min_element(cand.begin(), cand.end())->value;
      b[1] = std::max_element(cand.begin(), cand.end())->value;
      f_min = b[0];
      std::vector<double> ct;
      thrust.computeMinMaxMagnitudeCandidateTimes(0, 0.0, T, kXYZ, &ct);
      for (size_t i = 0; i < ct.size() && (int)i < cap; ++i) cand_times[(size_t)s * 2 * cap + i] = ct[i];
    }
    if (set(2)) {
      std::vector<mtg::Extremum> cand;
      seg.computeMinMaxMagnitudeCandidates(mtg::derivative_order::VELOCITY, 0.0, T, kXYZ, &cand);
      b[2] = std::max_element(cand.begin(), cand.end())->value;
    }
    if (set(3)) {
      std::vector<mtg::Extremum> cand;
      seg.computeMinMaxMagnitudeCandidates(mtg::derivative_order::JERK, 0.0, T, kXYZ, &cand);
      const double j_max = std::max_element(cand.begin(), cand.end())->value;
      b[3] = f_min > 1.0e-6 ? std::sqrt(j_max / f_min) : std::numeric_limits<double>::max();
      std::vector<double> ct;
      seg.computeMinMaxMagnitudeCandidateTimes(mtg::derivative_order::JERK, 0.0, T, kXYZ, &ct);
      for (size_t i = 0; i < ct.size() && (int)i < cap; ++i) cand_times[(size_t)s * 2 * cap + cap + i] = ct[i];
    }
    if (dim == 4) {
      std::pair<double, double> mn, mx;
      if (set(4)) {
        seg[3].computeMinMax(0.0, T, mtg::derivative_order::ANGULAR_VELOCITY, &mn, &mx);
        b[4] = std::max(std::abs(mn.second), std::abs(mx.second));
      }
      if (set(5)) {
        seg[3].computeMinMax(0.0, T, mtg::derivative_order::ANGULAR_ACCELERATION, &mn, &mx);
        b[5] = std::max(std::abs(mn.second), std::abs(mx.second));
      }
    }
  }
}

}  // extern "C"
"""


def build_wrapper(tmp):
    for rel, text in STAND_INS.items():
        path = os.path.join(tmp, "stand_in", rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
    wrap = os.path.join(tmp, "feasibility_wrap.cpp")
    with open(wrap, "w") as f:
        f.write(WRAPPER)
    core, ros = os.path.join(REF, "mav_trajectory_generation"), os.path.join(REF, "mav_trajectory_generation_ros")
    srcs = [os.path.join(core, "src", f) for f in ("polynomial.cpp", "vertex.cpp", "segment.cpp", "trajectory.cpp", "motion_defines.cpp",
                                                   "rpoly/rpoly_ak1.cpp")]
    srcs += [os.path.join(ros, "src", f) for f in ("feasibility_analytic.cpp", "input_constraints.cpp")]
    lib = os.path.join(tmp, "libfeasibility_ref.so")
    subprocess.check_call(["g++", "-O2", "-DNDEBUG", "-std=c++17", "-fPIC", "-w", "-shared", "-I" + os.path.join(tmp, "stand_in"),
                           "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + os.path.join(core, "include"),
                           "-I" + os.path.join(ros, "include"), "-o", lib, wrap] + srcs)
    so = ctypes.CDLL(lib)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    so.fz_make.argtypes = [ctypes.c_int] * 3 + [ctypes.c_double] * 3 + [ctypes.c_ulonglong, dp, dp]
    so.fz_check.argtypes = [ctypes.c_int] * 3 + [dp, dp, dp, ctypes.c_double, ip, ip]
    so.fz_bounds.argtypes = [ctypes.c_int] * 3 + [dp, dp, dp, dp, dp, ctypes.c_int]
    return so


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def limits_of(**kw):
    names = ("f_min", "f_max", "v_max", "omega_xy_max", "omega_z_max", "omega_z_dot_max")
    assert set(kw) <= set(names)
    return np.array([abs(kw[n]) if n in kw else NAN for n in names])


DEFAULTS = dict(f_min=0.5 * G, f_max=1.5 * G, v_max=3.0, omega_xy_max=math.pi / 2, omega_z_max=math.pi / 2, omega_z_dot_max=2 * math.pi)

# name, N, K, D, box, (v, a) of estimateSegmentTimes, B, first seed, [(limit set name, limits, min_section_time_s)]
CASES = [
    ("n10_k8_d3_slow", 10, 8, 3, 10.0, (2.0, 2.0), 100, 1, [
        ("defaults", limits_of(**DEFAULTS), 0.05),
        ("defaults_fine", limits_of(**dict(DEFAULTS, omega_xy_max=0.6)), 0.01)]),
    ("n10_k8_d3_thrust", 10, 8, 3, 10.0, (3.0, 4.0), 100, 1, [
        ("thrust", limits_of(f_min=8.5, f_max=11.0), 0.05),
        ("thrust_low", limits_of(f_min=9.0), 0.05),
        ("thrust_high", limits_of(f_max=10.6), 0.05)]),
    ("n10_k8_d3_fast", 10, 8, 3, 10.0, (8.0, 30.0), 100, 1, [
        ("roll_pitch", limits_of(omega_xy_max=1.0), 0.05),
        ("roll_pitch_fine", limits_of(omega_xy_max=0.8), 0.01),
        ("no_velocity", limits_of(f_min=0.5 * G, f_max=1.5 * G), 0.05)]),
    ("n10_k2_d3", 10, 2, 3, 5.0, (3.0, 6.0), 150, 1, [
        ("defaults", limits_of(**DEFAULTS), 0.05)]),
    ("n12_k1_d4", 12, 1, 4, 5.0, (3.0, 6.0), 200, 1, [
        ("yaw_rate", limits_of(omega_z_max=1.2), 0.05),
        ("yaw_acc", limits_of(omega_z_dot_max=1.5), 0.05)]),
    ("n12_k4_d4", 12, 4, 4, 5.0, (3.0, 6.0), 60, 1, [
        ("all_six", limits_of(f_min=4.9, f_max=14.7, v_max=3.0, omega_xy_max=1.57, omega_z_max=1.57, omega_z_dot_max=6.28), 0.05),
        ("yaw_acc", limits_of(omega_z_dot_max=1.5), 0.05)]),
]


def check_batch(so, n, k, dim, coeffs, times, limits, min_section):
    bsz = coeffs.shape[0]
    seg = np.zeros((bsz, k), dtype=np.int32)
    traj = np.zeros((bsz,), dtype=np.int32)
    first = np.zeros((bsz,), dtype=np.int32)
    f = ctypes.c_int(0)
    lim = np.ascontiguousarray(limits, dtype=np.float64)
    for b in range(bsz):
        row = np.zeros((k,), dtype=np.int32)
        traj[b] = so.fz_check(n, k, dim, _dp(coeffs[b]), _dp(times[b]), _dp(lim), min_section,
                              row.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.byref(f))
        seg[b], first[b] = row, f.value
    return seg, traj, first


def split_margin(cand_times, T, min_section):
    """min over the candidate times of the distance to the nearest INTERIOR split point, in units of T."""
    if not T > min_section:
        return np.inf
    depth = max(0, int(math.ceil(math.log2(T / min_section))))
    if depth == 0:
        return np.inf
    m = 2 ** depth
    t = cand_times[np.isfinite(cand_times)]
    x = t / T * m
    j = np.clip(np.rint(x), 1, m - 1)
    return float(np.min(np.abs(x - j)) / m) if t.size else np.inf


def main():
    assert os.path.exists(os.path.join(REF, "mav_trajectory_generation_ros", "src", "feasibility_analytic.cpp")), "needs /root/reference"
    seen, later = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        so = build_wrapper(tmp)
        for name, n, k, dim, box, (v, a), bsz, seed0, sets in CASES:
            coeffs = np.zeros((bsz, k, dim, n))
            times = np.zeros((bsz, k))
            for b in range(bsz):
                assert so.fz_make(n, k, dim, box, v, a, seed0 + b, _dp(coeffs[b]), _dp(times[b])) == 0
            out = {"coeffs": coeffs, "times": times, "limit_sets": np.array([s[0] for s in sets])}
            for sname, limits, min_section in sets:
                t0 = time.perf_counter()
                seg, traj, first = check_batch(so, n, k, dim, coeffs, times, limits, min_section)
                per_traj_us = (time.perf_counter() - t0) / bsz * 1e6
                robust = np.ones((bsz,), dtype=bool)
                for scale in (1.0 - 1e-6, 1.0 + 1e-6):
                    seg_s, _, _ = check_batch(so, n, k, dim, coeffs, times, limits * scale, min_section)
                    robust &= (seg_s == seg).all(axis=1)
                cap = 2 * n + 2
                bounds = np.zeros((bsz, k, 6))
                cand = np.zeros((bsz, k, 2, cap))
                for b in range(bsz):
                    so.fz_bounds(n, k, dim, _dp(coeffs[b]), _dp(times[b]), _dp(np.ascontiguousarray(limits)), _dp(bounds[b]), _dp(cand[b]), cap)
                if np.isfinite(limits[3]):
                    for b in range(bsz):
                        for s in range(k):
                            if split_margin(cand[b, s].ravel(), times[b, s], min_section) < 1e-8:
                                robust[b] = False
                n_bad = int((~robust).sum())
                assert n_bad <= 0.01 * bsz and n_bad <= max(1, bsz // 100), (name, sname, n_bad)
                assert 5 not in seg
                out[f"{sname}/limits"], out[f"{sname}/min_section_time_s"] = limits, np.float64(min_section)
                out[f"{sname}/segment_result"], out[f"{sname}/trajectory_result"], out[f"{sname}/first_failing_segment"] = seg, traj, first
                out[f"{sname}/segment_bounds"], out[f"{sname}/robust"] = bounds, robust
                mix = {int(c): int((traj == c).sum()) for c in np.unique(traj)}
                for c, cnt in mix.items():
                    seen[c] = seen.get(c, 0) + cnt
                    later[c] = later.get(c, 0) + int(((traj == c) & (first > 0)).sum())
                print(f"{name}/{sname}: verdicts {mix}, non-robust {n_bad}, reference {per_traj_us:.0f} us per trajectory (check only)")
            path = os.path.join(HERE, f"reference_feasibility_{name}.npz")
            np.savez_compressed(path, **out)
            size = os.path.getsize(path)
            print(f"  wrote {path} ({size} B)")
            assert size <= 300 * 1000, size
    print("trajectory verdicts over the set:", seen, "with a failing segment that is not the first:", later)
    for code in (0, 1, 2, 3, 4, 6, 7):
        assert seen.get(code, 0) >= 5, code
        if code != 0:
            assert later.get(code, 0) >= 1, code
    assert 5 not in seen


if __name__ == "__main__":
    sys.exit(main())
