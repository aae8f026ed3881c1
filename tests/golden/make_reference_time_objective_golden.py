#!/usr/bin/env python3
"""Generates tests/golden/reference_time_objective_*.npz: values of the REFERENCE's own nonlinear time objective
(PolynomialOptimizationNonLinear<N>::objectiveFunctionTime / objectiveFunctionTimeAndConstraints,
impl/polynomial_optimization_nonlinear_impl.h:556-615, :660-742) with maximum-magnitude soft constraints (:767-795).

Build container only (needs /root/reference).  This script writes a C wrapper -- this project's own text, below -- to a temporary
directory, compiles it there together with the six core sources of oracle/Makefile's REF_SRCS from the reference tree where they
lie, with -I oracle/ref_shim (the Eigen / glog container stand-ins every other anchor here uses) and -I oracle/ref_shim_nlopt (the
TYPES-ONLY nlopt stand-in: the callbacks never touch nlopt), runs the cases and commits ONLY DATA.  Nothing compiled from the
reference is kept, nothing is written under oracle/.  The callbacks are private static members: the wrapper reaches them by
including the reference's nonlinear header with `private` spelt `public`, the trick of oracle/ref_nonlinear_wrap.cpp.

Inputs: tests/helpers.reference_batch (the bit-exact restatement of createRandomVertices + estimateSegmentTimesNfabian), the
segment times then multiplied by the case's scales (trajectory b uses scales[b % len(scales)]).

Per case: n, d, masks, times [B][K], d_fixed [B][D][n_fixed], time_cost_kind, time_penalty, use_soft_constraints,
soft_constraint_weight, maximum_cost, con_derivative [C], con_value [C]; the reference's total [B], components [B][3]
(cost_trajectory, cost_time, cost_soft_constraints of optimization_info_), maxima [B][C] (optimization_info_.maxima; with soft
constraints off, computeMaximumOfMagnitude called directly), and coeffs_ref [B][K][D][N], the reference's OWN coefficients after
the callback (the CPU test feeds these bits to the host form).  free-form case: also d_free [B][D][n_free], the reference's
solution perturbed, which the callback was given.

Robustness: a soft term is compared in its exponent, within  weight * (max_ref / limit) * delta  (delta = the maxima tolerance:
1e-9, for jerk +1e-6 upwards).  A term whose reference exponent lies within that band of ln(maximum_cost) could be capped on one
side only and is not compared; the share of such terms on the committed fixtures is 0 -- asserted here and again by the tests.
If a case breaches that, change its scales, not the rule.

search case: 32 trajectories; the pattern-search loop of mav_trajectory_generation_amd.pattern_search_segment_times run on the
reference's callback (same candidates, same selection rule): initial [B], candidates_objective [n_iterations][2K+1][B],
first_accept_iteration [B] (-1: none), first_accept_improvement [B] (relative), final_objective [B], final_times [B][K].
Also reference_time_objective_veneer_rows.txt: six trajectories of the first case as text, for the C++ veneer test.

Run from the repository root:   python tests/golden/make_reference_time_objective_golden.py
"""
import ctypes
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WRAPPER = r"""
#include <algorithm>
#include <cmath>
#include <cstring>
#include <iostream>
#include <limits>
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <tuple>
#include <vector>
#include <nlopt.hpp>
#include <mav_trajectory_generation/polynomial_optimization_linear.h>
#include <mav_trajectory_generation/trajectory.h>
#include <mav_trajectory_generation/vertex.h>
#define private public
#include <mav_trajectory_generation/polynomial_optimization_nonlinear.h>
#undef private

namespace mtg = mav_trajectory_generation;

namespace {
// out: total, cost_trajectory, cost_time, cost_soft_constraints, then one maximum per constraint
template <int N>
int objective_one(int deriv, int k, int dim, const int* masks, const double* times, const double* d_fixed, int n_fixed, int kind,
                  double time_penalty, int use_soft, double weight, int n_con, const int* con_der, const double* con_val,
                  const double* d_free_in, double* out, double* coeffs, double* d_free_out) {
  mtg::Vertex::Vector vertices(k + 1, mtg::Vertex(dim));
  int col = 0;
  for (int v = 0; v <= k; ++v)
    for (int p = 0; p < N / 2; ++p)
      if ((masks[v] >> p) & 1) {
        Eigen::VectorXd value(dim);
        for (int d = 0; d < dim; ++d) value[d] = d_fixed[(size_t)d * n_fixed + col];
        vertices[v].addConstraint(p, value);
        ++col;
      }
  mtg::NonlinearOptimizationParameters params;
  params.time_alloc_method = (mtg::NonlinearOptimizationParameters::TimeAllocMethod)kind;
  params.time_penalty = time_penalty;
  params.use_soft_constraints = use_soft != 0;
  params.soft_constraint_weight = weight;
  mtg::PolynomialOptimizationNonLinear<N> opt(dim, params);
  std::vector<double> t(times, times + k);
  opt.setupFromVertices(vertices, t, deriv);
  for (int q = 0; q < n_con; ++q) opt.addMaximumMagnitudeConstraint(con_der[q], con_val[q]);
  const int n_free = (int)opt.poly_opt_.getNumberFreeConstraints();
  std::vector<double> no_gradient;
  if (d_free_in) {
    std::vector<double> x(t);
    for (int d = 0; d < dim; ++d)
      for (int i = 0; i < n_free; ++i) x.push_back(d_free_in[(size_t)d * n_free + i]);
    out[0] = mtg::PolynomialOptimizationNonLinear<N>::objectiveFunctionTimeAndConstraints(x, no_gradient, &opt);
  } else {
    out[0] = mtg::PolynomialOptimizationNonLinear<N>::objectiveFunctionTime(t, no_gradient, &opt);
  }
  out[1] = opt.optimization_info_.cost_trajectory;
  out[2] = opt.optimization_info_.cost_time;
  out[3] = opt.optimization_info_.cost_soft_constraints;
  for (int q = 0; q < n_con; ++q)
    out[4 + q] = use_soft ? opt.optimization_info_.maxima[con_der[q]].value
                          : opt.poly_opt_.computeMaximumOfMagnitude(con_der[q], nullptr).value;
  mtg::Segment::Vector segments;
  opt.poly_opt_.getSegments(&segments);
  for (int s = 0; s < k; ++s)
    for (int d = 0; d < dim; ++d) {
      const Eigen::VectorXd c = segments[s][d].getCoefficients(0);
      for (int j = 0; j < N; ++j) coeffs[((size_t)s * dim + d) * N + j] = c[j];
    }
  if (d_free_out) {
    std::vector<Eigen::VectorXd> fc;
    opt.poly_opt_.getFreeConstraints(&fc);
    for (int d = 0; d < dim; ++d)
      for (int i = 0; i < n_free; ++i) d_free_out[(size_t)d * n_free + i] = fc[d][i];
  }
  return n_free;
}
}  // namespace

extern "C" int to_objective(int n, int deriv, int k, int dim, const int* masks, const double* times, const double* d_fixed, int n_fixed,
                            int kind, double time_penalty, int use_soft, double weight, int n_con, const int* con_der,
                            const double* con_val, const double* d_free_in, double* out, double* coeffs, double* d_free_out) {
#define TO_CASE(NN) case NN: return objective_one<NN>(deriv, k, dim, masks, times, d_fixed, n_fixed, kind, time_penalty, use_soft, weight, \
                                                     n_con, con_der, con_val, d_free_in, out, coeffs, d_free_out)
  switch (n) {
    TO_CASE(8);
    TO_CASE(10);
    TO_CASE(12);
    default: return -2;
  }
}
"""

SQUARED, RICHTER, SQUARED_C, RICHTER_C = 0, 1, 3, 4
MAXIMUM_COST = 1.0e12   # the default argument of evaluateMaximumMagnitudeAsSoftConstraint, which the callbacks never override


def build_wrapper(tmp):
    wrap = os.path.join(tmp, "time_objective_wrap.cpp")
    with open(wrap, "w") as f:
        f.write(WRAPPER)
    core = os.path.join(REF, "mav_trajectory_generation")
    srcs = [os.path.join(core, "src", f) for f in ("polynomial.cpp", "vertex.cpp", "segment.cpp", "trajectory.cpp", "motion_defines.cpp",
                                                   "rpoly/rpoly_ak1.cpp")]
    lib = os.path.join(tmp, "libtime_objective_ref.so")
    subprocess.check_call(["g++", "-O2", "-DNDEBUG", "-std=c++17", "-fPIC", "-pthread", "-w", "-shared",
                           "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + os.path.join(ROOT, "oracle", "ref_shim_nlopt"),
                           "-I" + os.path.join(core, "include"), "-o", lib, wrap] + srcs)
    so = ctypes.CDLL(lib)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    so.to_objective.argtypes = [ctypes.c_int] * 4 + [ip, dp, dp, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                                                     ctypes.c_double, ctypes.c_int, ip, dp, dp, dp, dp, dp]
    return so


def _dp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


class Problem:
    def __init__(self, so, n, d, masks, dim, kind, penalty, use_soft, weight, constraints):
        self.so, self.n, self.d, self.dim = so, n, d, dim
        self.masks = np.array(masks, dtype=np.int32)
        self.k = len(masks) - 1
        self.n_fixed = sum(bin(m).count("1") for m in masks)
        self.n_free = (self.k + 1) * (n // 2) - self.n_fixed
        self.kind, self.penalty, self.use_soft, self.weight = kind, penalty, use_soft, weight
        self.con_der = np.array([c[0] for c in constraints], dtype=np.int32)
        self.con_val = np.array([c[1] for c in constraints], dtype=np.float64)

    def evaluate(self, times, d_fixed, d_free_in=None, want_free=False):
        """One trajectory: (out [4 + C], coeffs [K][D][N], d_free [D][n_free] or None)."""
        out = np.zeros(4 + len(self.con_der))
        coeffs = np.zeros((self.k, self.dim, self.n))
        d_free = np.zeros((self.dim, max(self.n_free, 1))) if want_free else None
        times = np.ascontiguousarray(times, dtype=np.float64)
        d_fixed = np.ascontiguousarray(d_fixed, dtype=np.float64)
        if d_free_in is not None:
            d_free_in = np.ascontiguousarray(d_free_in, dtype=np.float64)
        rc = self.so.to_objective(self.n, self.d, self.k, self.dim, _ip(self.masks), _dp(times), _dp(d_fixed), self.n_fixed, self.kind,
                                  self.penalty, int(self.use_soft), self.weight, len(self.con_der), _ip(self.con_der), _dp(self.con_val),
                                  _dp(d_free_in), _dp(out), _dp(coeffs), _dp(d_free))
        assert rc == self.n_free, rc
        return out, coeffs, (d_free[:, :self.n_free] if want_free else None)


def maxima_delta(derivative):
    """(downwards, upwards) relative tolerance of a maximum: helpers.assert_extrema_close."""
    return (1e-9, 1e-9) if derivative in (1, 2) else (1e-9, 1e-6)


def near_cap_share(maxima, con_der, con_val, weight, maximum_cost, device_tol=0.0):
    """Share of soft terms whose reference exponent lies within the comparison band of ln(maximum_cost).  device_tol: the
    coefficient parity of the device tests (their maxima tolerance is twice that, plus that much more upwards for jerk)."""
    n_near = n_all = 0
    for q, (der, val) in enumerate(zip(con_der, con_val)):
        expo = weight * (maxima[:, q] / val - 1.0)
        lo, up = maxima_delta(int(der))
        if device_tol:
            lo, up = (2 * device_tol, 2 * device_tol) if der in (1, 2) else (2 * device_tol, up + device_tol)
        band = weight * (maxima[:, q] / val) * max(lo, up)
        n_near += int((np.abs(expo - math.log(maximum_cost)) <= band).sum())
        n_all += maxima.shape[0]
    return n_near / max(n_all, 1)


FIVE = (0.8, 0.9, 1.0, 1.1, 1.25)
VA = [(1, 3.0), (2, 5.0)]
# name, N, d, K, D, interior mask, trajectories, seed, scales, kind, use_soft, constraints, free form
CASES = [
    ("n10_k8_d3_squared", 10, 4, 8, 3, 1, 60, 4100, FIVE, SQUARED, True, VA, False),
    ("n10_k8_d3_richter", 10, 4, 8, 3, 1, 60, 4200, FIVE, RICHTER, True, VA, False),
    ("n10_k8_d3_soft_off", 10, 4, 8, 3, 1, 30, 4300, FIVE, SQUARED, False, VA, False),
    ("n10_k1_d3", 10, 4, 1, 3, 1, 60, 4400, FIVE, SQUARED, True, VA, False),
    ("n10_k16_d4_config5", 10, 4, 16, 4, 7, 30, 4500, FIVE, SQUARED, True, VA, False),
    ("n12_k4_d4", 12, 5, 4, 4, 1, 60, 4600, FIVE, SQUARED, True, VA, False),
    ("n10_k8_d3_jerk", 10, 4, 8, 3, 1, 60, 4700, FIVE, SQUARED, True, [(1, 3.0), (2, 5.0), (3, 12.0)], False),
    ("n10_k8_d3_free", 10, 4, 8, 3, 1, 40, 4800, FIVE, SQUARED_C, True, VA, True),
]
PENALTY, WEIGHT = 500.0, 100.0   # NonlinearOptimizationParameters' defaults


def run_case(so, case):
    import helpers
    name, n, d, k, dim, interior, bsz, seed, scales, kind, use_soft, constraints, free_form = case
    masks = helpers.masks_ends_full(n, k, interior)
    masks, times, d_fixed = helpers.reference_batch(bsz, k, n, dim, seed, masks)
    times = times * np.array([scales[b % len(scales)] for b in range(bsz)])[:, None]
    prob = Problem(so, n, d, masks, dim, kind, PENALTY, use_soft, WEIGHT, constraints)
    nc = len(constraints)
    total, comp, maxima = np.zeros(bsz), np.zeros((bsz, 3)), np.zeros((bsz, nc))
    coeffs = np.zeros((bsz, k, dim, n))
    d_free = np.zeros((bsz, dim, prob.n_free)) if free_form else None
    rng = np.random.default_rng(seed)
    for b in range(bsz):
        given = None
        if free_form:   # the reference's own optimum, perturbed: what an optimiser over (times, free constraints) hands the callback
            _, _, opt_free = prob.evaluate(times[b], d_fixed[b], want_free=True)
            given = opt_free * (1.0 + 0.02 * rng.standard_normal(opt_free.shape)) + 0.01 * rng.standard_normal(opt_free.shape)
            d_free[b] = given
        out, coeffs[b], _ = prob.evaluate(times[b], d_fixed[b], d_free_in=given)
        total[b], comp[b], maxima[b] = out[0], out[1:4], out[4:]
    assert np.isfinite(total).all() and np.isfinite(maxima).all()
    share = near_cap_share(maxima, prob.con_der, prob.con_val, WEIGHT, MAXIMUM_COST)
    assert share == 0.0, (name, share)
    device_tol = 5e-8 if n == 12 else 1e-9          # tol_for(n, d) of tests/test_gpu_vs_reference.py for d = N/2 - 1
    assert near_cap_share(maxima, prob.con_der, prob.con_val, WEIGHT, MAXIMUM_COST, device_tol) == 0.0, name
    data = dict(n=n, d=d, masks=np.array(masks, dtype=np.int64), times=times, d_fixed=d_fixed, time_cost_kind=kind, time_penalty=PENALTY,
                use_soft_constraints=int(use_soft), soft_constraint_weight=WEIGHT, maximum_cost=MAXIMUM_COST,
                con_derivative=prob.con_der.astype(np.int64), con_value=prob.con_val, total=total, components=comp, maxima=maxima,
                coeffs_ref=coeffs)
    if free_form:
        data["d_free"] = d_free
    with np.errstate(over="ignore"):
        terms = np.minimum(MAXIMUM_COST, np.exp(WEIGHT * (maxima / prob.con_val - 1.0)))
    print(f"{name}: soft terms {terms.min():.3g} .. {terms.max():.3g}, capped {int((terms >= MAXIMUM_COST).sum())} of {terms.size}, "
          f"near the cap {share:.0%}")
    return data, terms


def candidates(cur, step, lower_bound):
    """[2K + 1][K] candidates of one trajectory (mav_trajectory_generation_amd.pattern_search_segment_times)."""
    k = cur.shape[0]
    out = [cur.copy()]
    for j in range(k):
        c = cur.copy()
        c[j] = cur[j] * (1.0 + step)
        out.append(c)
    for j in range(k):
        c = cur.copy()
        c[j] = max(lower_bound, cur[j] * (1.0 - step))
        out.append(c)
    return np.array(out)


def run_search(so, n_iterations=12, step0=0.1, lower_bound=0.1):
    import helpers
    n, d, k, dim, bsz, seed = 10, 4, 8, 3, 32, 4900
    masks = helpers.masks_ends_full(n, k, 1)
    masks, times, d_fixed = helpers.reference_batch(bsz, k, n, dim, seed, masks)
    prob = Problem(so, n, d, masks, dim, SQUARED, PENALTY, True, WEIGHT, VA)
    nc = 2 * k + 1
    cand_obj = np.zeros((n_iterations, nc, bsz))
    initial, final_obj = np.zeros(bsz), np.zeros(bsz)
    first_it, first_impr = np.full(bsz, -1, dtype=np.int64), np.zeros(bsz)
    final_times = np.zeros((bsz, k))
    for b in range(bsz):
        cur, step = times[b].copy(), step0
        for it in range(n_iterations):
            cand = candidates(cur, step, lower_bound)
            obj = np.array([prob.evaluate(c, d_fixed[b])[0][0] for c in cand])
            cand_obj[it, :, b] = obj
            if it == 0:
                initial[b] = obj[0]
            j = int(np.argmin(obj[1:]))
            best = j + 1 if obj[1 + j] < obj[0] else 0
            if best and first_it[b] < 0:
                first_it[b], first_impr[b] = it, (obj[0] - obj[best]) / abs(obj[0])
            cur = cand[best]
            if best == 0:
                step *= 0.5
        final_times[b] = cur
        final_obj[b] = prob.evaluate(cur, d_fixed[b])[0][0]
    print(f"search: first accepted iteration {np.bincount(first_it + 1)}, improved by more than 1e-6: {int((first_impr > 1e-6).sum())} of {bsz}, "
          f"final / initial {np.median(final_obj / initial):.3f} (median)")
    return dict(n=n, d=d, masks=np.array(masks, dtype=np.int64), times=times, d_fixed=d_fixed, time_cost_kind=SQUARED, time_penalty=PENALTY,
                use_soft_constraints=1, soft_constraint_weight=WEIGHT, maximum_cost=MAXIMUM_COST,
                con_derivative=prob.con_der.astype(np.int64), con_value=prob.con_val, n_iterations=n_iterations, step0=step0,
                lower_bound=lower_bound, initial=initial, candidates_objective=cand_obj, first_accept_iteration=first_it,
                first_accept_improvement=first_impr, final_objective=final_obj, final_times=final_times)


def write_veneer_rows(data, n_rows=6):
    """tests/golden/reference_time_objective_veneer_rows.txt: a few trajectories of a case as text, for the C++ veneer test
    (tests/cpp/test_objective_veneer.cpp reads its reference-derived numbers from here instead of compiling them in)."""
    path = os.path.join(HERE, "reference_time_objective_veneer_rows.txt")
    bsz, k, dim, n = data["coeffs_ref"].shape
    fmt = lambda a: " ".join("%.17g" % x for x in np.asarray(a, dtype=np.float64).ravel())
    with open(path, "w") as f:
        f.write("# N K D rows constraints / (derivative value)... / weight maximum_cost / per row: times, coeffs [K][D][N], maxima, cost_soft\n")
        f.write(f"{n} {k} {dim} {n_rows} {len(data['con_value'])}\n")
        f.write(" ".join(f"{int(d)} {v:.17g}" for d, v in zip(data["con_derivative"], data["con_value"])) + "\n")
        f.write(f"{data['soft_constraint_weight']:.17g} {data['maximum_cost']:.17g}\n")
        for b in range(n_rows):
            f.write(fmt(data["times"][b]) + "\n" + fmt(data["coeffs_ref"][b]) + "\n" + fmt(data["maxima"][b]) + "\n" +
                    fmt(data["components"][b, 2]) + "\n")
    print(f"  wrote {path} ({os.path.getsize(path)} B)")


def main():
    assert os.path.exists(os.path.join(REF, "mav_trajectory_generation", "include", "mav_trajectory_generation",
                                       "polynomial_optimization_nonlinear.h")), "needs /root/reference"
    all_terms = []
    with tempfile.TemporaryDirectory() as tmp:
        so = build_wrapper(tmp)
        outputs = []
        for case in CASES:
            data, terms = run_case(so, case)
            outputs.append((case[0], data))
            if case[10]:
                all_terms.append(terms.ravel())
        outputs.append(("search", run_search(so)))
    for name, data in outputs:
        path = os.path.join(HERE, f"reference_time_objective_{name}.npz")
        np.savez_compressed(path, **data)
        size = os.path.getsize(path)
        print(f"  wrote {path} ({size} B)")
        assert size <= 240 * 1000, size
    write_veneer_rows(dict(outputs)["n10_k8_d3_squared"])
    terms = np.concatenate(all_terms)
    # the whole range: far below one, around one, and the cap
    assert terms.min() < 1e-6 and (terms >= MAXIMUM_COST).sum() >= 5 and ((terms > 0.1) & (terms < 1e6)).sum() >= 5, (terms.min(), terms.max())


if __name__ == "__main__":
    sys.exit(main())
