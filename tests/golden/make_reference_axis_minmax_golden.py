#!/usr/bin/env python3
"""Generates tests/golden/reference_axis_minmax_*.npz: per-axis signed extrema from the REFERENCE's own
Polynomial::computeMinMax(0, T, q, &min, &max) (src/polynomial.cpp:102-143, Jenkins-Traub below it).

Build container only (needs /root/reference).  Like make_reference_half_plane_golden.py, this script writes a C wrapper -- this
project's own text, below -- to a temporary directory, compiles there the six core sources of oracle/Makefile's REF_SRCS from the
reference tree where they lie, with -I oracle/ref_shim, runs the cases and commits ONLY DATA.  Nothing compiled from the
reference is kept, nothing is written under oracle/.

Inputs.  The coefficients and times ALREADY COMMITTED are read, not regenerated: reference_feasibility_{n10_k2_d3,
n10_k8_d3_fast, n12_k1_d4, n12_k4_d4}.npz, and the odd-N `coeffs` / `times` of reference_half_plane_{n5_k3_d3, n7_k4_d4}.npz.

Per case: `minmax` [B'][K][D][orders][4] = (t_min, v_min, t_max, v_max) for q = 0 .. min(4, N - 1), and `n_trajectories` = B'.
B' is the whole fixture except for n10_k8_d3_fast, which stores its first 40 trajectories (the 250 000 B limit of a file).

Asserted here, and again by tests/test_axis_minmax.py: interior extrema (a time that is neither 0 nor T) occur, as minima and
as maxima, in every (case, order) that can have them -- all but the linear and constant orders 3 and 4 of n5_k3_d3.

The files are written with fixed zip timestamps: a second run reproduces them bit for bit.

Run from the repository root:   python tests/golden/make_reference_axis_minmax_golden.py
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

WRAPPER = r"""
#include <mav_trajectory_generation/polynomial.h>

#include <utility>

namespace mtg = mav_trajectory_generation;

extern "C" {

// Polynomial::computeMinMax(0, T, q) for q = 0 .. n_orders - 1 on count polynomials of n coefficients (increasing powers),
// polynomial i with time times[i]; out[i][q] = (t_min, v_min, t_max, v_max).  Returns the number of calls that returned false.
int am_minmax(int n, long long count, const double* coeffs, const double* times, int n_orders, double* out) {
  int failed = 0;
  for (long long i = 0; i < count; ++i) {
    Eigen::VectorXd c(n);
    for (int j = 0; j < n; ++j) c[j] = coeffs[i * n + j];
    const mtg::Polynomial p(n, c);
    for (int q = 0; q < n_orders; ++q) {
      std::pair<double, double> lo, hi;
      if (!p.computeMinMax(0.0, times[i], q, &lo, &hi)) ++failed;
      double* o = out + (i * n_orders + q) * 4;
      o[0] = lo.first; o[1] = lo.second; o[2] = hi.first; o[3] = hi.second;
    }
  }
  return failed;
}

}  // extern "C"
"""


def build_wrapper(tmp):
    wrap = os.path.join(tmp, "axis_minmax_wrap.cpp")
    with open(wrap, "w") as f:
        f.write(WRAPPER)
    core = os.path.join(REF, "mav_trajectory_generation")
    srcs = [os.path.join(core, "src", f) for f in ("polynomial.cpp", "vertex.cpp", "segment.cpp", "trajectory.cpp", "motion_defines.cpp",
                                                   "rpoly/rpoly_ak1.cpp")]
    lib = os.path.join(tmp, "libaxis_minmax_ref.so")
    subprocess.check_call(["g++", "-O2", "-DNDEBUG", "-std=c++17", "-fPIC", "-w", "-shared", "-I" + os.path.join(ROOT, "oracle", "ref_shim"),
                           "-I" + os.path.join(core, "include"), "-o", lib, wrap] + srcs)
    so = ctypes.CDLL(lib)
    dp = ctypes.POINTER(ctypes.c_double)
    so.am_minmax.argtypes = [ctypes.c_int, ctypes.c_longlong, dp, dp, ctypes.c_int, dp]
    return so


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


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


def interior_counts(minmax, times):
    """[orders][2]: rows whose minimum / maximum lies strictly inside (0, T)."""
    T = times[:, :, None, None]
    return np.stack([((minmax[..., 0] != 0.0) & (minmax[..., 0] != T)).sum(axis=(0, 1, 2)),
                     ((minmax[..., 2] != 0.0) & (minmax[..., 2] != T)).sum(axis=(0, 1, 2))], axis=1)


# name, committed source of (coeffs, times), trajectories stored (None: all)
CASES = [
    ("n10_k2_d3", "reference_feasibility_n10_k2_d3.npz", None),
    ("n10_k8_d3_fast", "reference_feasibility_n10_k8_d3_fast.npz", 40),
    ("n12_k1_d4", "reference_feasibility_n12_k1_d4.npz", None),
    ("n12_k4_d4", "reference_feasibility_n12_k4_d4.npz", None),
    ("n5_k3_d3", "reference_half_plane_n5_k3_d3.npz", None),
    ("n7_k4_d4", "reference_half_plane_n7_k4_d4.npz", None),
]


def main():
    assert os.path.exists(os.path.join(REF, "mav_trajectory_generation", "src", "polynomial.cpp")), "needs /root/reference"
    with tempfile.TemporaryDirectory() as tmp:
        so = build_wrapper(tmp)
        for name, source, keep in CASES:
            z = np.load(os.path.join(HERE, source))
            coeffs, times = z["coeffs"], z["times"]
            if keep is not None:
                coeffs, times = coeffs[:keep], times[:keep]
            coeffs, times = np.ascontiguousarray(coeffs, dtype=np.float64), np.ascontiguousarray(times, dtype=np.float64)
            bsz, k, dim, n = coeffs.shape
            orders = min(4, n - 1) + 1
            per_poly_T = np.ascontiguousarray(np.broadcast_to(times[:, :, None], (bsz, k, dim)))
            minmax = np.zeros((bsz, k, dim, orders, 4))
            failed = so.am_minmax(n, bsz * k * dim, _dp(coeffs), _dp(per_poly_T), orders, _dp(minmax))
            assert failed == 0, (name, failed)
            cnt = interior_counts(minmax, times)
            for q in range(orders):
                can = n - q - 2 >= 1   # p^(q+1) is at least linear
                print(f"{name} order {q}: interior minima {cnt[q, 0]}, interior maxima {cnt[q, 1]} of {bsz * k * dim}")
                assert (cnt[q, 0] > 0 and cnt[q, 1] > 0) == can, (name, q, cnt[q])
            path = os.path.join(HERE, f"reference_axis_minmax_{name}.npz")
            save_deterministic(path, {"minmax": minmax, "n_trajectories": np.int64(bsz)})
            size = os.path.getsize(path)
            print(f"  wrote {path} ({size} B)")
            assert size <= 250 * 1000, size


if __name__ == "__main__":
    sys.exit(main())
