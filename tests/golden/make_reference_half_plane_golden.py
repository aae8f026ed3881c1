#!/usr/bin/env python3
"""Generates tests/golden/reference_half_plane_*.npz: half-plane verdicts and clearances from the REFERENCE's own
Polynomial::computeMinMaxCandidates and Segment::evaluate on trajectories its own solveLinear() produced.

Build container only (needs /root/reference).  Like make_reference_feasibility_golden.py, this script writes a C wrapper -- this
project's own text, below -- to a temporary directory, compiles there the six core sources of oracle/Makefile's REF_SRCS from the
reference tree where they lie, with -I oracle/ref_shim, runs the cases and commits ONLY DATA.  Nothing compiled from the
reference is kept, nothing is written under oracle/.

What is and is not the reference's code.  mav_trajectory_generation_ros/src/feasibility_base.cpp is tried first
(reference_unit_compiles below): it does not compile against the unchanged Eigen stand-in of oracle/ref_shim (head(3), cross,
normalized, normalize, finished are members the stand-in's matrix class lacks, and members cannot be supplied from outside the
class), so, as for the input check's first-failing-segment loop, the loop over segments, planes and candidates in hp_check is
this generator's own lines, written against the reference's public API:
    projection = sum_dim segment[dim] * normal[dim]            (Polynomial::operator*, operator+=: the reference's)
    projection.computeMinMaxCandidates(0, T, POSITION, &cand)  (the reference's, Jenkins-Traub below it)
    clearance(t) = (segment.evaluate(t)[0..2] - point) . normal, summed in the order x, y, z   (Segment::evaluate: the reference's)
    a plane fails iff some candidate has clearance <= 0.0; the first failing plane and segment are the first in loop order.
Unlike the reference's loop, hp_check does not return at the first failure: it records the minimum clearance over every
plane and candidate.  The verdicts are those of the early-returning loop by construction.

Inputs.  The coefficients and times ALREADY COMMITTED in reference_feasibility_{n10_k2_d3, n10_k8_d3_fast, n12_k1_d4,
n12_k4_d4}.npz are read, not regenerated.  Two odd-N cases anchor the zero-padding: the reference's PolynomialOptimization<N>
accepts even N only (static_assert), so n5_k3_d3 / n7_k4_d4 are its solveLinear() solutions for N = 6 / 8 with the
highest-power coefficient dropped -- polynomials of 5 / 7 coefficients that start at the same vertices; their coeffs and times
are stored in their files.

Plane sets, per case: bounding boxes centred at the origin with edge 16, 20, 22, 26 (HalfPlane::createBoundingBox's order and
signs), the oblique pair point (0, 0, -8) / normal (0.3, -0.2, 1) and point (5, 0, 0) / normal (-1, 0.5, 0.2), and for
n10_k2_d3 one per-segment corridor: box k of trajectory b is the bounding box of segment k's two end positions grown by
CORRIDOR_MARGIN = 0.75 on every side ([B][K][6][4]).  Planes are handed to the wrapper as (point, unit normal) and stored as
`s/planes` rows (nx, ny, nz, offset = point . n), the library's format.

Per set s: `s/planes`, `s/segment_feasible` [B][K] (bool), `s/trajectory_feasible` [B], `s/first_failing_segment` [B] (-1: none),
`s/first_failing_plane` [B] (-1: none), `s/segment_clearance` [B][K], `s/robust` [B].  reference_half_plane_veneer_rows.txt: eight
trajectories of n10_k8_d3_fast with their box22 / oblique verdicts as text, for the C++ veneer's test program.

robust: the reference's per-segment verdicts and first failing planes are unchanged with every plane moved along its normal by
+ and by - 1e-9 * max(1, |offset|).  The cap on non-robust trajectories is 0 for every set here: asserted below and again
by the tests.  If a set breaches it, change the plane set (or the corridor margin), not the cap.

The files are written with fixed zip timestamps: a second run reproduces them bit for bit.

Run from the repository root:   python tests/golden/make_reference_half_plane_golden.py
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
CORRIDOR_MARGIN = 0.75

STAND_INS = {
    "ros/ros.h": "#pragma once\n#define ROS_ERROR_STREAM(x) do { } while (0)\n#define ROS_WARN_STREAM(x) do { } while (0)\n"
                 "#define ROS_INFO_STREAM(x) do { } while (0)\n#define ROS_DEBUG_STREAM(x) do { } while (0)\n",
    "mav_msgs/default_values.h": "#pragma once\nnamespace mav_msgs { const double kGravity = 9.81; }\n",
    "yaml-cpp/yaml.h": "#pragma once\n#include <string>\nnamespace YAML {\nstruct Node {\n  Node operator[](const std::string&) const { return Node(); }\n"
                       "  template <class T> Node& operator=(const T&) { return *this; }\n  template <class T> T as() const { return T(); }\n"
                       "  explicit operator bool() const { return false; }\n};\n}\n",
    "Eigen/Geometry": "#pragma once\n#include <Eigen/Core>\n",
    "Eigen/StdVector": "#pragma once\n#include <Eigen/Core>\n#ifndef EIGEN_MAKE_ALIGNED_OPERATOR_NEW\n"
                       "#define EIGEN_MAKE_ALIGNED_OPERATOR_NEW\n#endif\n",
}

WRAPPER = r"""
#include <mav_trajectory_generation/polynomial_optimization_linear.h>
#include <mav_trajectory_generation/trajectory.h>
#include <mav_trajectory_generation/vertex.h>

#include <cmath>
#include <limits>
#include <vector>

namespace mtg = mav_trajectory_generation;

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

// solveLinear() for N coefficients; the first `keep` of each polynomial are written (keep = N - 1: the odd-N cases)
template <int N>
int make_one(int keep, int k, int dim, double box, double v, double a, unsigned long long seed, double* coeffs, double* times) {
  const int derivative = N / 2 - 1;
  const mtg::Vertex::Vector vertices = mtg::createRandomVertices(derivative, k, Eigen::VectorXd::Constant(dim, -box),
                                                                 Eigen::VectorXd::Constant(dim, box), seed);
  const std::vector<double> segment_times = mtg::estimateSegmentTimes(vertices, v, a);
  mtg::PolynomialOptimization<N> opt(dim);
  opt.setupFromVertices(vertices, segment_times, derivative);
  opt.solveLinear();
  mtg::Segment::Vector segments;
  opt.getSegments(&segments);
  for (int s = 0; s < k; ++s) {
    times[s] = segments[s].getTime();
    for (int d = 0; d < dim; ++d) {
      const Eigen::VectorXd c = segments[s][d].getCoefficients(0);
      for (int j = 0; j < keep; ++j) coeffs[((size_t)s * dim + d) * keep + j] = c[j];
    }
  }
  return 0;
}

}  // namespace

extern "C" {

int hp_make(int n_solve, int keep, int k, int dim, double box, double v, double a, unsigned long long seed, double* coeffs,
            double* times) {
  switch (n_solve) {
    case 6: return make_one<6>(keep, k, dim, box, v, a, seed, coeffs, times);
    case 8: return make_one<8>(keep, k, dim, box, v, a, seed, coeffs, times);
    default: return -1;
  }
}

// One trajectory.  Segment s uses the n_planes planes at points / normals + s * stride (stride in planes; 0: one set).
// Returns 1 if every segment passes; *first_segment / *first_plane: the first failure in loop order, -1 if none.
int hp_check(int n, int k, int dim, const double* coeffs, const double* times, const double* points, const double* normals,
             int n_planes, int stride, int* segment_feasible, int* segment_first_plane, double* segment_clearance,
             int* first_segment, int* first_plane) {
  *first_segment = -1;
  *first_plane = -1;
  for (int s = 0; s < k; ++s) {
    const mtg::Segment seg = make_segment(n, dim, coeffs + (size_t)s * dim * n, times[s]);
    segment_feasible[s] = 1;
    segment_first_plane[s] = -1;
    segment_clearance[s] = std::numeric_limits<double>::infinity();
    if (!(seg.D() == 3 || seg.D() == 4)) {
      segment_feasible[s] = 0;
      segment_clearance[s] = std::numeric_limits<double>::quiet_NaN();
    } else {
      for (int h = 0; h < n_planes; ++h) {
        const double* pt = points + ((size_t)s * stride + h) * 3;
        const double* nr = normals + ((size_t)s * stride + h) * 3;
        mtg::Polynomial projection(seg.N());
        for (int d = 0; d < 3; ++d) projection += seg[d] * nr[d];
        std::vector<double> candidates;
        projection.computeMinMaxCandidates(0.0, seg.getTime(), mtg::derivative_order::POSITION, &candidates);
        for (double t : candidates) {
          const Eigen::VectorXd pos = seg.evaluate(t);
          const double clearance = (pos[0] - pt[0]) * nr[0] + (pos[1] - pt[1]) * nr[1] + (pos[2] - pt[2]) * nr[2];
          if (clearance <= 0.0 && segment_first_plane[s] < 0) {
            segment_feasible[s] = 0;
            segment_first_plane[s] = h;
          }
          if (clearance < segment_clearance[s]) segment_clearance[s] = clearance;
        }
      }
    }
    if (!segment_feasible[s] && *first_segment < 0) {
      *first_segment = s;
      *first_plane = segment_first_plane[s];
    }
  }
  return *first_segment < 0 ? 1 : 0;
}

}  // extern "C"
"""


def _write_stand_ins(tmp):
    for rel, text in STAND_INS.items():
        path = os.path.join(tmp, "stand_in", rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)


def _includes(tmp):
    core, ros = os.path.join(REF, "mav_trajectory_generation"), os.path.join(REF, "mav_trajectory_generation_ros")
    return ["-I" + os.path.join(tmp, "stand_in"), "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + os.path.join(core, "include"),
            "-I" + os.path.join(ros, "include")]


def reference_unit_compiles(tmp):
    """feasibility_base.cpp itself against oracle/ref_shim and the stand-ins above: does it compile?"""
    src = os.path.join(REF, "mav_trajectory_generation_ros", "src", "feasibility_base.cpp")
    r = subprocess.run(["g++", "-O0", "-std=c++17", "-fPIC", "-w", "-fsyntax-only"] + _includes(tmp) + [src], capture_output=True, text=True)
    return r.returncode == 0, r.stderr


def build_wrapper(tmp):
    wrap = os.path.join(tmp, "half_plane_wrap.cpp")
    with open(wrap, "w") as f:
        f.write(WRAPPER)
    core = os.path.join(REF, "mav_trajectory_generation")
    srcs = [os.path.join(core, "src", f) for f in ("polynomial.cpp", "vertex.cpp", "segment.cpp", "trajectory.cpp", "motion_defines.cpp",
                                                   "rpoly/rpoly_ak1.cpp")]
    lib = os.path.join(tmp, "libhalf_plane_ref.so")
    subprocess.check_call(["g++", "-O2", "-DNDEBUG", "-std=c++17", "-fPIC", "-w", "-shared"] + _includes(tmp) + ["-o", lib, wrap] + srcs)
    so = ctypes.CDLL(lib)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    so.hp_make.argtypes = [ctypes.c_int] * 4 + [ctypes.c_double] * 3 + [ctypes.c_ulonglong, dp, dp]
    so.hp_check.argtypes = [ctypes.c_int] * 3 + [dp, dp, dp, dp, ctypes.c_int, ctypes.c_int, ip, ip, dp, ip, ip]
    return so


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def box_points_normals(center, size):
    """HalfPlane::createBoundingBox: per axis (bbx_min, +e) then (bbx_max, -e)."""
    center, size = np.asarray(center, dtype=np.float64), np.asarray(size, dtype=np.float64)
    lo, hi = center - size / 2.0, center + size / 2.0
    pts, nrm = [], []
    for axis in range(3):
        e = np.zeros(3)
        e[axis] = 1.0
        pts += [lo, hi]
        nrm += [e, -e + 0.0]   # (-1, 0, 0) with positive zeros, as normal_max(axis) = -1.0 on a zero vector gives
    return np.array(pts), np.array(nrm)


def unit(normals):
    normals = np.asarray(normals, dtype=np.float64)
    return normals / np.sqrt((normals * normals).sum(axis=-1, keepdims=True))   # (HalfPlane's constructor: normal.normalize())


def planes_of(points, normals):
    return np.concatenate([normals, (points * normals).sum(axis=-1, keepdims=True)], axis=-1)


OBLIQUE_NORMALS = [[0.3, -0.2, 1.0], [-1.0, 0.5, 0.2]]
OBLIQUE = (np.array([[0.0, 0.0, -8.0], [5.0, 0.0, 0.0]]), unit(OBLIQUE_NORMALS))


def write_veneer_rows(path, coeffs, times, out, edge=22, n_each=4):
    """Text rows for tests/cpp/test_half_plane_veneer.cpp: the first n_each feasible and n_each infeasible trajectories under the
    box of that edge, with the reference's verdicts for the box and the oblique pair (normals as given, not normalised)."""
    feas = out[f"box{edge}/trajectory_feasible"]
    pick = sorted(list(np.flatnonzero(feas == 1)[:n_each]) + list(np.flatnonzero(feas == 0)[:n_each]))
    _, k, dim, n = coeffs.shape
    with open(path, "w") as f:
        f.write("# N K D rows box_edge / oblique (point, normal) x 2 / per row: times, coefficients [K][D][N], box segment verdicts, "
                "oblique segment verdicts, box verdict, oblique verdict, box first failing segment, box first failing plane\n")
        f.write(f"{n} {k} {dim} {len(pick)} {edge}\n")
        for pt, nr in zip(OBLIQUE[0], OBLIQUE_NORMALS):
            f.write(" ".join(repr(float(v)) for v in list(pt) + list(nr)) + "\n")
        for b in pick:
            f.write(" ".join(repr(float(v)) for v in times[b]) + "\n")
            for s in range(k):
                for d in range(dim):
                    f.write(" ".join(repr(float(v)) for v in coeffs[b, s, d]) + "\n")
            f.write(" ".join(str(int(v)) for v in out[f"box{edge}/segment_feasible"][b]) + "\n")
            f.write(" ".join(str(int(v)) for v in out["oblique/segment_feasible"][b]) + "\n")
            f.write(f"{int(feas[b])} {int(out['oblique/trajectory_feasible'][b])} {int(out[f'box{edge}/first_failing_segment'][b])} "
                    f"{int(out[f'box{edge}/first_failing_plane'][b])}\n")


def shared_sets():
    sets = [(f"box{edge}", *box_points_normals((0.0, 0.0, 0.0), (edge,) * 3)) for edge in (16, 20, 22, 26)]
    sets.append(("oblique", *OBLIQUE))
    return sets


def corridor_set(coeffs, times, margin):
    """[B][K][6] points and normals: box k = bounding box of segment k's end positions, grown by `margin` on every side."""
    bsz, k, _, n = coeffs.shape
    pts, nrm = np.zeros((bsz, k, 6, 3)), np.zeros((bsz, k, 6, 3))
    for b in range(bsz):
        for s in range(k):
            p0 = coeffs[b, s, :3, 0]
            p1 = np.array([np.polyval(coeffs[b, s, d, ::-1], times[b, s]) for d in range(3)])
            lo, hi = np.minimum(p0, p1) - margin, np.maximum(p0, p1) + margin
            pts[b, s], nrm[b, s] = box_points_normals((lo + hi) / 2.0, hi - lo)
    return pts, nrm


def check_batch(so, coeffs, times, points, normals):
    bsz, k, dim, n = coeffs.shape
    per_traj = points.ndim == 4
    n_planes = points.shape[-2]
    seg = np.zeros((bsz, k), dtype=np.int32)
    seg_plane = np.zeros((bsz, k), dtype=np.int32)
    clear = np.zeros((bsz, k))
    traj = np.zeros((bsz,), dtype=np.int32)
    fseg = np.zeros((bsz,), dtype=np.int32)
    fplane = np.zeros((bsz,), dtype=np.int32)
    a, c = ctypes.c_int(0), ctypes.c_int(0)
    for b in range(bsz):
        pt = np.ascontiguousarray(points[b] if per_traj else points)
        nr = np.ascontiguousarray(normals[b] if per_traj else normals)
        row, rowp, rowc = np.zeros((k,), dtype=np.int32), np.zeros((k,), dtype=np.int32), np.zeros((k,))
        traj[b] = so.hp_check(n, k, dim, _dp(np.ascontiguousarray(coeffs[b])), _dp(np.ascontiguousarray(times[b])), _dp(pt), _dp(nr),
                              n_planes, n_planes if per_traj else 0, _ip(row), _ip(rowp), _dp(rowc), ctypes.byref(a), ctypes.byref(c))
        seg[b], seg_plane[b], clear[b], fseg[b], fplane[b] = row, rowp, rowc, a.value, c.value
    return seg, seg_plane, clear, traj, fseg, fplane


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


# name, source of (coeffs, times): a committed feasibility fixture, or (N solved, K, D, box, (v, a), B, first seed) for an odd-N case
CASES = [
    ("n10_k2_d3", "reference_feasibility_n10_k2_d3.npz", True),
    ("n10_k8_d3_fast", "reference_feasibility_n10_k8_d3_fast.npz", False),
    ("n12_k1_d4", "reference_feasibility_n12_k1_d4.npz", False),
    ("n12_k4_d4", "reference_feasibility_n12_k4_d4.npz", False),
    ("n5_k3_d3", (6, 3, 3, 6.0, (8.0, 30.0), 40, 1), False),
    ("n7_k4_d4", (8, 4, 4, 6.0, (8.0, 30.0), 40, 1), False),
]


def main():
    assert os.path.exists(os.path.join(REF, "mav_trajectory_generation", "src", "polynomial.cpp")), "needs /root/reference"
    verdicts = {}
    with tempfile.TemporaryDirectory() as tmp:
        _write_stand_ins(tmp)
        ok, err = reference_unit_compiles(tmp)
        print("feasibility_base.cpp against oracle/ref_shim:", "COMPILES -- use it instead of hp_check's own loop" if ok else
              "does not compile (" + next((l for l in err.splitlines() if "error" in l), "?").strip()[:150] + "); the plane loop is the generator's")
        so = build_wrapper(tmp)
        for name, source, with_corridor in CASES:
            out = {}
            if isinstance(source, str):
                z = np.load(os.path.join(HERE, source))
                coeffs, times = z["coeffs"], z["times"]
            else:
                n_solve, k, dim, box, (v, a), bsz, seed0 = source
                keep = n_solve - 1
                coeffs, times = np.zeros((bsz, k, dim, keep)), np.zeros((bsz, k))
                for b in range(bsz):
                    assert so.hp_make(n_solve, keep, k, dim, box, v, a, seed0 + b, _dp(coeffs[b]), _dp(times[b])) == 0
                out["coeffs"], out["times"] = coeffs, times
            bsz = coeffs.shape[0]
            sets = shared_sets()
            if with_corridor:
                sets.append(("corridor", *corridor_set(coeffs, times, CORRIDOR_MARGIN)))
            out["plane_sets"] = np.array([s[0] for s in sets])
            for sname, points, normals in sets:
                seg, seg_plane, clear, traj, fseg, fplane = check_batch(so, coeffs, times, points, normals)
                planes = planes_of(points, normals)
                robust = np.ones((bsz,), dtype=bool)
                delta = 1e-9 * np.maximum(1.0, np.abs(planes[..., 3:4]))
                for sign in (-1.0, 1.0):   # offset' = offset + sign * delta  <=>  point' = point + sign * delta * n
                    seg_s, seg_plane_s, _, _, _, _ = check_batch(so, coeffs, times, points + sign * delta * normals, normals)
                    robust &= (seg_s == seg).all(axis=1) & (seg_plane_s == seg_plane).all(axis=1)
                n_bad = int((~robust).sum())
                assert n_bad == 0, (name, sname, n_bad)
                out[f"{sname}/planes"] = planes
                out[f"{sname}/segment_feasible"] = seg.astype(bool)
                out[f"{sname}/trajectory_feasible"] = traj
                out[f"{sname}/first_failing_segment"], out[f"{sname}/first_failing_plane"] = fseg, fplane
                out[f"{sname}/segment_clearance"], out[f"{sname}/robust"] = clear, robust
                verdicts[(name, sname)] = (int(traj.sum()), bsz)
                print(f"{name}/{sname}: feasible {int(traj.sum())}/{bsz}, failing not in segment 0: {int((fseg > 0).sum())}, "
                      f"smallest |clearance| {np.abs(clear).min():.2e}, non-robust {n_bad}")
            if name == "n10_k8_d3_fast":
                write_veneer_rows(os.path.join(HERE, "reference_half_plane_veneer_rows.txt"), coeffs, times, out)
            path = os.path.join(HERE, f"reference_half_plane_{name}.npz")
            save_deterministic(path, out)
            size = os.path.getsize(path)
            print(f"  wrote {path} ({size} B)")
            assert size <= 250 * 1000, size
    # both verdicts occur, and failures that are not in the first segment
    assert 0 < verdicts[("n10_k8_d3_fast", "box20")][0] < 100 and 0 < verdicts[("n10_k8_d3_fast", "box26")][0] < 100
    assert 0 < verdicts[("n10_k2_d3", "corridor")][0] < verdicts[("n10_k2_d3", "corridor")][1]


if __name__ == "__main__":
    sys.exit(main())
