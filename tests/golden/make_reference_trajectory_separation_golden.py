#!/usr/bin/env python3
"""Generates tests/golden/reference_trajectory_separation_*.npz: distances between pairs of trajectories over the time both fly,
from the REFERENCE's own Segment::computeMinMaxMagnitudeCandidates and Segment::evaluate on trajectories its own solveLinear()
produced.

Build container only (needs /root/reference).  Like make_reference_recursive_feasibility_golden.py, this script writes a C wrapper
-- this project's own text, below -- to a temporary directory, compiles there the six core sources of oracle/Makefile's REF_SRCS
from the reference tree where they lie, with -I oracle/ref_shim, runs the cases and commits ONLY DATA.  Nothing compiled from the
reference is kept, nothing is written under oracle/.

What is and is not the reference's code.  The reference has no check of one trajectory against another.  Per piece (a stretch of
time between two merged breakpoints, on which both trajectories are one polynomial each) ts_piece below uses its public API:
    Segment::computeMinMaxMagnitudeCandidates(POSITION, 0, L, {0, 1, 2}, &candidates)   on the DIFFERENCE segment (the reference's,
                                                                                         Jenkins-Traub below it): candidate times
    Segment::evaluate(sa + x), Segment::evaluate(sb + x)                                 on the two ORIGINAL segments (the
                                                                                         reference's): the positions there
The generator's own lines: the breakpoints (one float64 addition per step) and the pieces, the coefficients of the difference
segment (both sides shifted to the piece's start by the binomial expansion in np.longdouble, subtracted, rounded to float64), the
two ends of the piece added to the candidates, the norm of the difference of the two positions over dimensions 0-2, the minimum
over the candidates (the first on a tie), the fold over the pieces in time order, the verdict `distance - min_separation > 0` and
the first-failure bookkeeping.

Inputs.  The coefficients and times ALREADY COMMITTED are read, not regenerated: reference_feasibility_{n10_k8_d3_fast, n10_k2_d3,
n12_k4_d4}.npz and reference_half_plane_n7_k4_d4.npz.  Per file numpy.random.default_rng(20261100 + index of the case): 60 pairs
(a, b), a != b, of trajectories of that file, drawn first; then a start time per trajectory uniform in [0, 2].  min_separation is
the median of the 60 pair distances rounded to three decimals, so that both verdicts occur.

Per case: `pairs` [P][2], `start` [B], `min_separation`, `distance` [P] (the minimum; +inf without a piece), `closest_time` [P]
(global), `closest_segment_a` / `_b` [P], `pair_feasible` [P], `first_failing_segment_a` / `_b` [P] (-1: none), `robust` [P],
`scale` [P] (min_separation + the reference's max ||p|| of both trajectories), `piece_pair`, `piece_a`, `piece_b`, `piece_distance`
(every piece of every pair, in time order).  reference_trajectory_separation_veneer_rows.txt: eight pairs of n10_k8_d3_fast with
their results as text, for the C++ veneer's test program.

robust (per pair): the verdict and the first failing piece are unchanged with min_separation times 1 + 1e-6 and times 1 - 1e-6.
At most max(1, P // 100) pairs may be non-robust, and each verdict must occur at least five times: asserted below.  If a case
breaches that, change the seed, not the cap.

The files are written with fixed zip timestamps: a second run reproduces them bit for bit.

Run from the repository root:   python tests/golden/make_reference_trajectory_separation_golden.py
"""
import ctypes
import io
import math
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
N_PAIRS = 60

WRAPPER = r"""
#include <mav_trajectory_generation/segment.h>

#include <cmath>
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

}  // namespace

extern "C" {

// One piece of length L: diff = [3][n] coefficients of the difference in the time since the piece's start; a, b = the ORIGINAL
// segments ([dim][n]) of times ta, tb, whose local times at the piece's start are sa, sb.  *distance: the smallest
// ||a(sa + x) - b(sb + x)|| over x = 0, L and the reference's candidates (the first on a tie), *x_min: that x.
int ts_piece(int n, int dim, const double* diff, double L, const double* a, double ta, double sa, const double* b, double tb, double sb,
             double* distance, double* x_min) {
  const std::vector<int> dims = {0, 1, 2};
  std::vector<mtg::Extremum> candidates;
  if (!make_segment(n, 3, diff, L).computeMinMaxMagnitudeCandidates(mtg::derivative_order::POSITION, 0.0, L, dims, &candidates)) return -1;
  std::vector<double> x = {0.0, L};
  for (const mtg::Extremum& c : candidates)
    if (c.time >= 0.0 && c.time <= L) x.push_back(c.time);
  const mtg::Segment seg_a = make_segment(n, dim, a, ta), seg_b = make_segment(n, dim, b, tb);
  *distance = INFINITY;
  *x_min = 0.0;
  for (double v : x) {
    const Eigen::VectorXd pa = seg_a.evaluate(sa + v), pb = seg_b.evaluate(sb + v);
    double acc = 0.0;
    for (int d = 0; d < 3; ++d) acc += (pa[d] - pb[d]) * (pa[d] - pb[d]);
    const double dist = std::sqrt(acc);
    if (dist < *distance) { *distance = dist; *x_min = v; }
  }
  return 0;
}

// maximum of ||p|| over one segment (the reference's candidates and selection)
int ts_max_position(int n, int dim, const double* coeffs, double t, double* out) {
  const std::vector<int> dims = {0, 1, 2};
  const mtg::Segment seg = make_segment(n, dim, coeffs, t);
  std::vector<mtg::Extremum> candidates;
  mtg::Extremum minimum, maximum;
  if (!seg.computeMinMaxMagnitudeCandidates(mtg::derivative_order::POSITION, 0.0, t, dims, &candidates)) return -1;
  if (!seg.selectMinMaxMagnitudeFromCandidates(mtg::derivative_order::POSITION, 0.0, t, dims, candidates, &minimum, &maximum)) return -1;
  *out = maximum.value;
  return 0;
}

}  // extern "C"
"""


def build_wrapper(tmp):
    wrap = os.path.join(tmp, "trajectory_separation_wrap.cpp")
    with open(wrap, "w") as f:
        f.write(WRAPPER)
    core = os.path.join(REF, "mav_trajectory_generation")
    srcs = [os.path.join(core, "src", f) for f in ("polynomial.cpp", "vertex.cpp", "segment.cpp", "trajectory.cpp", "motion_defines.cpp",
                                                   "rpoly/rpoly_ak1.cpp")]
    lib = os.path.join(tmp, "libtrajectory_separation_ref.so")
    subprocess.check_call(["g++", "-O2", "-DNDEBUG", "-std=c++17", "-fPIC", "-w", "-shared", "-I" + os.path.join(ROOT, "oracle", "ref_shim"),
                           "-I" + os.path.join(core, "include"), "-o", lib, wrap] + srcs)
    so = ctypes.CDLL(lib)
    dp, d = ctypes.POINTER(ctypes.c_double), ctypes.c_double
    so.ts_piece.argtypes = [ctypes.c_int, ctypes.c_int, dp, d, dp, d, d, dp, d, d, dp, dp]
    so.ts_max_position.argtypes = [ctypes.c_int, ctypes.c_int, dp, d, dp]
    return so


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def breakpoints(times, start):
    e = [np.float64(start)]
    for t in times:
        e.append(np.float64(e[-1] + np.float64(t)))
    return e


def shifted(c, s):
    """[3][N] longdouble coefficients of p(s + x) in x; c [D][N] float64."""
    n = c.shape[1]
    out = np.zeros((3, n), dtype=LD)
    for k in range(n):
        for i in range(k + 1):
            out[:, i] += LD(math.comb(k, i)) * c[:3, k].astype(LD) * LD(s) ** (k - i)
    return out


def pair_pieces(so, ca, ta, start_a, cb, tb, start_b):
    """[(i, j, distance, global time)] of one pair in time order."""
    ea, eb = breakpoints(ta, start_a), breakpoints(tb, start_b)
    dim, n = ca.shape[1:]
    out = []
    for rank in range(len(ta) + len(tb) - 1):
        for i in range(len(ta)):
            j = rank - i
            if j < 0 or j >= len(tb):
                continue
            lo, hi = max(ea[i], eb[j]), min(ea[i + 1], eb[j + 1])
            if not lo < hi:
                continue
            sa, sb, length = float(lo - ea[i]), float(lo - eb[j]), float(hi - lo)
            diff = np.ascontiguousarray((shifted(ca[i], sa) - shifted(cb[j], sb)).astype(np.float64))
            a, b = np.ascontiguousarray(ca[i]), np.ascontiguousarray(cb[j])
            dist, x = ctypes.c_double(0.0), ctypes.c_double(0.0)
            assert so.ts_piece(n, dim, _dp(diff), length, _dp(a), float(ta[i]), sa, _dp(b), float(tb[j]), sb, ctypes.byref(dist),
                               ctypes.byref(x)) == 0
            out.append((i, j, dist.value, float(lo + x.value)))
    return out


def fold(pieces, min_separation):
    best, when, ba, bb, first = math.inf, math.nan, -1, -1, (-1, -1)
    for i, j, dist, t in pieces:
        if dist < best:
            best, when, ba, bb = dist, t, i, j
        if first[0] < 0 and not (dist - min_separation > 0.0):
            first = (i, j)
    return best, when, ba, bb, first


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


def write_veneer_rows(path, coeffs, times, out, n_each=4):
    """Text rows for tests/cpp/test_trajectory_separation_veneer.cpp: the first n_each feasible and n_each infeasible robust pairs."""
    feas, robust = out["pair_feasible"], out["robust"]
    pick = sorted(list(np.flatnonzero((feas == 1) & robust)[:n_each]) + list(np.flatnonzero((feas == 0) & robust)[:n_each]))
    _, k, dim, n = coeffs.shape
    with open(path, "w") as f:
        f.write("# N K D rows min_separation / per row: for side a then side b: start, times, coefficients [K][D][N]; then verdict, first "
                "failing segment a, first failing segment b, separation, scale\n")
        f.write(f"{n} {k} {dim} {len(pick)} {float(out['min_separation'])!r}\n")
        for p in pick:
            for index in out["pairs"][p]:
                f.write(repr(float(out["start"][index])) + "\n")
                f.write(" ".join(repr(float(v)) for v in times[index]) + "\n")
                for s in range(k):
                    for d in range(dim):
                        f.write(" ".join(repr(float(v)) for v in coeffs[index, s, d]) + "\n")
            f.write(f"{int(feas[p])} {int(out['first_failing_segment_a'][p])} {int(out['first_failing_segment_b'][p])} "
                    f"{float(out['distance'][p] - out['min_separation'])!r} {float(out['scale'][p])!r}\n")


CASES = [("n10_k8_d3_fast", "reference_feasibility_n10_k8_d3_fast.npz"), ("n10_k2_d3", "reference_feasibility_n10_k2_d3.npz"),
         ("n12_k4_d4", "reference_feasibility_n12_k4_d4.npz"), ("n7_k4_d4", "reference_half_plane_n7_k4_d4.npz")]


def main():
    assert os.path.exists(os.path.join(REF, "mav_trajectory_generation", "src", "polynomial.cpp")), "needs /root/reference"
    with tempfile.TemporaryDirectory() as tmp:
        so = build_wrapper(tmp)
        for index, (name, source) in enumerate(CASES):
            z = np.load(os.path.join(HERE, source))
            coeffs, times = np.ascontiguousarray(z["coeffs"]), np.ascontiguousarray(z["times"])
            bsz, k, dim, n = coeffs.shape
            rng = np.random.default_rng(20261100 + index)
            a = rng.integers(bsz, size=N_PAIRS)
            b = (a + 1 + rng.integers(bsz - 1, size=N_PAIRS)) % bsz
            pairs = np.stack([a, b], axis=1).astype(np.int32)
            start = rng.uniform(0.0, 2.0, bsz)
            pmax = np.zeros(bsz)
            one = ctypes.c_double(0.0)
            for t in sorted(set(pairs.ravel().tolist())):
                for s in range(k):
                    assert so.ts_max_position(n, dim, _dp(np.ascontiguousarray(coeffs[t, s])), float(times[t, s]), ctypes.byref(one)) == 0
                    pmax[t] = max(pmax[t], one.value)
            pieces = [pair_pieces(so, coeffs[x], times[x], start[x], coeffs[y], times[y], start[y]) for x, y in pairs]
            msep = round(float(np.median([fold(p, 0.0)[0] for p in pieces])), 3)
            rows = [fold(p, msep) for p in pieces]
            feas = np.array([int(r[4][0] < 0) for r in rows], dtype=np.int32)
            robust = np.array([fold(p, msep * (1 - 1e-6))[4] == r[4] == fold(p, msep * (1 + 1e-6))[4] for p, r in zip(pieces, rows)])
            n_bad = int((~robust).sum())
            assert n_bad <= max(1, N_PAIRS // 100) and n_bad <= max(1.0, 0.01 * N_PAIRS), (name, n_bad)
            assert int(feas.sum()) >= 5 and int((feas == 0).sum()) >= 5, (name, int(feas.sum()))
            out = {"pairs": pairs, "start": start, "min_separation": np.float64(msep), "distance": np.array([r[0] for r in rows]),
                   "closest_time": np.array([r[1] for r in rows]), "closest_segment_a": np.array([r[2] for r in rows], dtype=np.int32),
                   "closest_segment_b": np.array([r[3] for r in rows], dtype=np.int32), "pair_feasible": feas,
                   "first_failing_segment_a": np.array([r[4][0] for r in rows], dtype=np.int32),
                   "first_failing_segment_b": np.array([r[4][1] for r in rows], dtype=np.int32), "robust": robust,
                   "scale": msep + pmax[pairs[:, 0]] + pmax[pairs[:, 1]],
                   "piece_pair": np.array([p for p, ps in enumerate(pieces) for _ in ps], dtype=np.int32),
                   "piece_a": np.array([q[0] for ps in pieces for q in ps], dtype=np.int32),
                   "piece_b": np.array([q[1] for ps in pieces for q in ps], dtype=np.int32),
                   "piece_distance": np.array([q[2] for ps in pieces for q in ps])}
            print(f"{name}: min_separation {msep}, feasible {int(feas.sum())}/{N_PAIRS}, pieces {len(out['piece_pair'])}, "
                  f"failing not in the first piece: {int(sum(r[4][0] + r[4][1] > 0 for r in rows))}, non-robust {n_bad}")
            if name == "n10_k8_d3_fast":
                write_veneer_rows(os.path.join(HERE, "reference_trajectory_separation_veneer_rows.txt"), coeffs, times, out)
            path = os.path.join(HERE, f"reference_trajectory_separation_{name}.npz")
            save_deterministic(path, out)
            size = os.path.getsize(path)
            print(f"  wrote {path} ({size} B)")
            assert size <= 300 * 1000, size


if __name__ == "__main__":
    sys.exit(main())
