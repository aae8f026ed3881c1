"""Thin object layer over the C ABI: Context (device, stream), Plan (N, K, D, d, masks), solve.

Mirrors the reference call sequence (polynomial_optimization_linear.h:57-108):
    PolynomialOptimization<N> opt(D); opt.setupFromVertices(vertices, times, d); opt.solveLinear();
as  plan = Plan(ctx, N, D, K, d, fixed_mask); plan.solve(times, d_fixed) -> coeffs [B][K][D][N]
for a whole batch of trajectories sharing the constraint structure.
torch is used only to own device memory and streams.
"""
from __future__ import annotations

import ctypes
import enum
from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import _lib as L

library_path = L.LIB_PATH


class MtgError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"mtg error {code}: {msg}")
        self.code = code


def _check(lib, code: int, ctx_handle=None):
    if code != 0:
        msg = lib.mtg_status_string(code).decode()
        if ctx_handle:
            extra = lib.mtg_last_error_string(ctx_handle).decode()
            if extra:
                msg += " (" + extra + ")"
        raise MtgError(code, msg)


class Context:
    """(device, stream, scratch).  Owns a torch.cuda.Stream (`.stream`) that the library enqueues on;
    solve calls are ordered after work already queued on torch's current stream and vice versa."""

    def __init__(self, device: int = 0, stream=None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("mav_trajectory_generation_amd needs a HIP device (a context always owns a GPU; batches have no CPU path)")
        self.lib = L.load()
        self.device = int(device)
        self.stream = stream if stream is not None else torch.cuda.Stream(self.device)
        h = ctypes.c_void_p()
        _check(self.lib, self.lib.mtg_context_create(self.device, ctypes.c_void_p(self.stream.cuda_stream),
                                                     ctypes.byref(h)))
        self.handle = h
        import os
        import weakref
        self._plans = weakref.WeakSet()   # plans must be destroyed before their context
        # measurement knobs (include/mtg_hip_lab.h): the library itself never reads the environment
        for env, (name, conv) in L.ENV_OPTIONS.items():
            if env in os.environ:
                self.set_option(name, conv(os.environ[env]))

    def set_option(self, name: str, value: int):
        """A measurement knob of this context by name (include/mtg_hip_lab.h: A/B runs and form-forcing tests)."""
        _check(self.lib, self.lib.mtg_context_set_option(self.handle, name.encode(), int(value)), self.handle)

    def lab_segment_cost_matrices(self, n_coeffs: int, derivative: int, times, variant: int):
        """EVIDENCE variant (include/mtg_hip_lab.h: mtg_lab_segment_cost_matrices): H_k = A_k^-T Q_k A_k^-1 (LIN:318) of the
        given segment times, [n][N][N]; variant 1 = literally on the FP64 matrix cores, 0 = the scaling identity."""
        import torch
        t = times.contiguous()
        out = torch.empty((t.numel(), n_coeffs, n_coeffs), dtype=torch.float64, device=t.device)
        cur = self._enter()
        try:
            _check(self.lib, self.lib.mtg_lab_segment_cost_matrices(self.handle, n_coeffs, derivative, t.numel(), t.data_ptr(),
                                                                    out.data_ptr(), variant), self.handle)
        finally:
            self._leave(cur)
        return out

    def clock_probe_start(self, duration_us: float):
        """Start a shader-clock probe (include/mtg_hip_lab.h: mtg_lab_clock_probe_start) next to whatever runs on the device for
        the next `duration_us`; returns the handle clock_probe_finish takes."""
        h = ctypes.c_void_p()
        _check(self.lib, self.lib.mtg_lab_clock_probe_start(self.handle, float(duration_us), ctypes.byref(h)), self.handle)
        return h

    def clock_probe_finish(self, probe):
        """(shader clock in MHz over the probed interval, the interval in us)."""
        mhz, us = ctypes.c_double(0), ctypes.c_double(0)
        _check(self.lib, self.lib.mtg_lab_clock_probe_finish(probe, ctypes.byref(mhz), ctypes.byref(us)), self.handle)
        return mhz.value, us.value

    def _enter(self):
        """Order the library's stream after torch's current stream (no-op when they are the same)."""
        import torch
        cur = torch.cuda.current_stream(self.device)
        if cur != self.stream:
            self.stream.wait_stream(cur)
        return cur

    def _leave(self, cur):
        if cur != self.stream:
            cur.wait_stream(self.stream)

    def sync(self):
        _check(self.lib, self.lib.mtg_context_sync(self.handle), self.handle)

    def compare_coefficients(self, a, b):
        """(max over polynomials of ||a - b||_inf / ||b||_inf, max |a - b|) of two coefficient tensors [..., N], computed on
        the device (C ABI: mtg_compare_coefficients).  Synchronous."""
        assert a.shape == b.shape and a.is_cuda and b.is_cuda and a.is_contiguous() and b.is_contiguous()
        n = a.shape[-1]
        rel, ab = ctypes.c_double(0), ctypes.c_double(0)
        cur = self._enter()
        rc = self.lib.mtg_compare_coefficients(self.handle, ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()),
                                               a.numel() // n, n, ctypes.byref(rel), ctypes.byref(ab))
        self._leave(cur)
        _check(self.lib, rc, self.handle)
        return rel.value, ab.value

    def selftest_rcp(self, n: int = 1 << 20) -> float:
        out = ctypes.c_double(0)
        _check(self.lib, self.lib.mtg_selftest_rcp(self.handle, n, ctypes.byref(out)), self.handle)
        return out.value

    def close(self):
        if getattr(self, "handle", None):
            for p in list(getattr(self, "_plans", ())):
                p.close()
            self.lib.mtg_context_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sample_range(ctx: "Context", coeffs, times, t_start: float, dt: float, n_samples: int, n_derivatives: int = 5,
                 times_layout: str = "aos", want_valid: bool = False, out=None, valid=None):
    """Batched Trajectory::evaluateRange / sampleTrajectoryInRange: coeffs [B][K][D][N] and times ([B][K] 'aos' or
    [K][B] 'soa') CUDA tensors -> out [B][n_samples][n_derivatives][D] (and n_valid [B] int32).
    `out` / `valid`: caller-owned result buffers (float64 / int32 CUDA tensors of exactly that many elements on the device of
    `coeffs`, contiguous, `out` 16-byte aligned) instead of fresh allocations; `valid` implies want_valid.  The results are
    views of them in the shapes above."""
    import torch
    bsz, k, dim, n = coeffs.shape
    assert coeffs.is_cuda and coeffs.dtype == torch.float64 and coeffs.is_contiguous() and times.is_contiguous()
    shape = (bsz, n_samples, n_derivatives, dim)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=coeffs.device)
    else:
        if not (out.is_cuda and out.device == coeffs.device and out.dtype == torch.float64):
            raise ValueError("sample_range: `out` must be a float64 tensor on the device of `coeffs`")
        if out.numel() != bsz * n_samples * n_derivatives * dim or not out.is_contiguous():
            raise ValueError("sample_range: `out` must be contiguous with %d x %d x %d x %d elements" % shape)
        if out.data_ptr() % 16:
            raise ValueError("sample_range: `out` must be 16-byte aligned")
        out = out.view(shape)
    if valid is None:
        valid = torch.empty((bsz,), dtype=torch.int32, device=coeffs.device) if want_valid else None
    else:
        if not (valid.is_cuda and valid.device == coeffs.device and valid.dtype == torch.int32):
            raise ValueError("sample_range: `valid` must be an int32 tensor on the device of `coeffs`")
        if valid.numel() != bsz or not valid.is_contiguous():
            raise ValueError("sample_range: `valid` must be contiguous with %d elements" % bsz)
        valid = valid.view((bsz,))
        want_valid = True
    sb, sk = (k, 1) if times_layout == "aos" else (1, bsz)
    cur = ctx._enter()
    rc = ctx.lib.mtg_sample_range(ctx.handle, n, k, dim, bsz, ctypes.c_void_p(coeffs.data_ptr()),
                                  ctypes.c_void_p(times.data_ptr()), sb, sk, float(t_start), float(dt), n_samples,
                                  n_derivatives, ctypes.c_void_p(out.data_ptr()),
                                  ctypes.c_void_p(valid.data_ptr()) if valid is not None else None)
    ctx._leave(cur)
    _check(ctx.lib, rc, ctx.handle)
    return (out, valid) if want_valid else out


def minmax_magnitude(ctx: "Context", coeffs, times, derivative: int, dimensions: Optional[Sequence[int]] = None,
                     times_layout: str = "aos"):
    """Batched Trajectory::computeMinMaxMagnitude: coeffs [B][K][D][N], times ([B][K] 'aos' / [K][B] 'soa') CUDA
    tensors -> (segment_minmax [B][K][4], trajectory_minmax [B][4], trajectory_segment_idx [B][2] int32); the four
    columns are (t_min, v_min, t_max, v_max) with segment-local times."""
    import torch
    bsz, k, dim, n = coeffs.shape
    assert coeffs.is_cuda and coeffs.dtype == torch.float64 and coeffs.is_contiguous() and times.is_contiguous()
    mask = 0
    for d in (dimensions if dimensions is not None else range(dim)):
        if d < 0 or d >= dim:
            raise MtgError(-1, "dimension %d out of bounds [0..%d]" % (d, dim - 1))
        mask |= 1 << d
    seg = torch.empty((bsz, k, 4), dtype=torch.float64, device=coeffs.device)
    traj = torch.empty((bsz, 4), dtype=torch.float64, device=coeffs.device)
    idx = torch.empty((bsz, 2), dtype=torch.int32, device=coeffs.device)
    sb, sk = (k, 1) if times_layout == "aos" else (1, bsz)
    cur = ctx._enter()
    rc = ctx.lib.mtg_minmax_magnitude(ctx.handle, n, k, dim, bsz, ctypes.c_void_p(coeffs.data_ptr()),
                                      ctypes.c_void_p(times.data_ptr()), sb, sk, int(derivative), mask,
                                      ctypes.c_void_p(seg.data_ptr()), ctypes.c_void_p(traj.data_ptr()),
                                      ctypes.c_void_p(idx.data_ptr()))
    ctx._leave(cur)
    _check(ctx.lib, rc, ctx.handle)
    return seg, traj, idx


class AxisMinMax(NamedTuple):
    """segment [B][K][D][n][4], trajectory [B][D][n][4] or None, trajectory_segment_idx [B][D][n][2] int32 or None; the four
    columns are (t_min, v_min, t_max, v_max) with segment-local times, n the orders asked for."""
    segment: object
    trajectory: object
    trajectory_segment_idx: object


def minmax_axes(ctx: "Context", coeffs, times, derivative_first: int = 0, n_derivatives: int = 1, times_layout: str = "aos",
                want_trajectory: bool = True) -> AxisMinMax:
    """Batched Polynomial::computeMinMax: the signed minimum and maximum of every axis over every segment, for the orders
    derivative_first .. derivative_first + n_derivatives - 1 (0 = position .. 4 = snap) from one root search per axis.  coeffs
    [B][K][D][N], times ([B][K] 'aos' / [K][B] 'soa') CUDA float64 tensors.  A row with a NaN candidate is (0, NaN, 0, NaN)."""
    import torch
    bsz, k, dim, n = coeffs.shape
    assert coeffs.is_cuda and coeffs.dtype == torch.float64 and coeffs.is_contiguous() and times.is_contiguous()
    nd = int(n_derivatives)
    if nd < 1 or nd > 5:
        raise MtgError(-1, "n_derivatives must be in [1, 5]")
    dev = coeffs.device
    seg = torch.empty((bsz, k, dim, nd, 4), dtype=torch.float64, device=dev)
    traj = torch.empty((bsz, dim, nd, 4), dtype=torch.float64, device=dev) if want_trajectory else None
    idx = torch.empty((bsz, dim, nd, 2), dtype=torch.int32, device=dev) if want_trajectory else None
    sb, sk = (k, 1) if times_layout == "aos" else (1, bsz)
    cur = ctx._enter()
    rc = ctx.lib.mtg_minmax_axes(ctx.handle, n, k, dim, bsz, ctypes.c_void_p(coeffs.data_ptr()), ctypes.c_void_p(times.data_ptr()),
                                 sb, sk, int(derivative_first), nd, ctypes.c_void_p(seg.data_ptr()),
                                 ctypes.c_void_p(traj.data_ptr()) if traj is not None else None,
                                 ctypes.c_void_p(idx.data_ptr()) if idx is not None else None)
    ctx._leave(cur)
    _check(ctx.lib, rc, ctx.handle)
    return AxisMinMax(seg, traj, idx)


def minmax_axes_host(coeffs, times, derivative_first: int = 0, n_derivatives: int = 1, times_layout: str = "aos",
                     want_trajectory: bool = True) -> AxisMinMax:
    """The same on numpy arrays through the library's host build of the same code (no context, no device): coeffs
    [B][K][D][N] or one trajectory [K][D][N] (then the results come without the batch axis)."""
    lib = L.load()
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    times = np.ascontiguousarray(times, dtype=np.float64)
    single = coeffs.ndim == 3
    if single:
        coeffs, times = coeffs[None], times[None]
    bsz, k, dim, n = coeffs.shape
    if times.size != bsz * k:
        raise MtgError(-1, "times must hold one value per segment")
    nd = int(n_derivatives)
    if nd < 1 or nd > 5:
        raise MtgError(-1, "n_derivatives must be in [1, 5]")
    seg = np.empty((bsz, k, dim, nd, 4), dtype=np.float64)
    traj = np.empty((bsz, dim, nd, 4), dtype=np.float64) if want_trajectory else None
    idx = np.empty((bsz, dim, nd, 2), dtype=np.int32) if want_trajectory else None
    sb, sk = (k, 1) if times_layout == "aos" else (1, bsz)
    rc = lib.mtg_minmax_axes_host(n, k, dim, bsz, coeffs.ctypes.data, times.ctypes.data, sb, sk, int(derivative_first), nd,
                                  seg.ctypes.data, traj.ctypes.data if traj is not None else None,
                                  idx.ctypes.data if idx is not None else None)
    _check(lib, rc)
    res = AxisMinMax(seg, traj, idx)
    return AxisMinMax(*[a if a is None else a[0] for a in res]) if single else res


def bounding_boxes(ctx: "Context", coeffs, times, times_layout: str = "aos", margin: float = 0.0):
    """Axis-aligned bounding boxes of position from one minmax_axes call of order 0: (segment_lo_hi [B][K][2][D],
    trajectory_lo_hi [B][2][D]), lo - margin / hi + margin."""
    import torch
    r = minmax_axes(ctx, coeffs, times, 0, 1, times_layout, True)
    seg = torch.stack([r.segment[:, :, :, 0, 1] - margin, r.segment[:, :, :, 0, 3] + margin], dim=2)
    traj = torch.stack([r.trajectory[:, :, 0, 1] - margin, r.trajectory[:, :, 0, 3] + margin], dim=1)
    return seg, traj


def scale_segment_times_to_meet_constraints(ctx: "Context", coeffs, times, v_max: float, a_max: float,
                                            max_iterations: int = 2, times_layout: str = "aos", workspace=None):
    """Batched Trajectory::scaleSegmentTimesToMeetConstraints, IN PLACE on coeffs [B][K][D][N] and times.
    Returns (scaling [B], within_range [B] int32, workspace); workspace[2*B*K*4:].view(2, B, 4)[:, :, 3] are the
    maximum |velocity| / |acceleration| seen by the last round's check."""
    import torch
    bsz, k, dim, n = coeffs.shape
    assert coeffs.is_cuda and coeffs.dtype == torch.float64 and coeffs.is_contiguous() and times.is_contiguous()
    need = 8 * bsz * (k + 1)
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.float64, device=coeffs.device)
    assert workspace.numel() >= need and workspace.dtype == torch.float64
    scaling = torch.empty((bsz,), dtype=torch.float64, device=coeffs.device)
    within = torch.empty((bsz,), dtype=torch.int32, device=coeffs.device)
    sb, sk = (k, 1) if times_layout == "aos" else (1, bsz)
    cur = ctx._enter()
    rc = ctx.lib.mtg_scale_segment_times_to_meet_constraints(
        ctx.handle, n, k, dim, bsz, ctypes.c_void_p(coeffs.data_ptr()), ctypes.c_void_p(times.data_ptr()), sb, sk,
        float(v_max), float(a_max), int(max_iterations), ctypes.c_void_p(workspace.data_ptr()),
        ctypes.c_void_p(scaling.data_ptr()), ctypes.c_void_p(within.data_ptr()))
    ctx._leave(cur)
    _check(ctx.lib, rc, ctx.handle)
    return scaling, within, workspace


class InputFeasibilityResult(enum.IntEnum):
    """The reference's enum InputFeasibilityResult (mav_trajectory_generation_ros feasibility_base.h:34-50)."""
    kInputFeasible = 0
    kInputIndeterminable = 1
    kInputInfeasibleThrustHigh = 2
    kInputInfeasibleThrustLow = 3
    kInputInfeasibleVelocity = 4
    kInputInfeasibleRollPitchRates = 5
    kInputInfeasibleYawRates = 6
    kInputInfeasibleYawAcc = 7


_RESULT_NAMES = ("Feasible", "Indeterminable", "InfeasibleThrustHigh", "InfeasibleThrustLow", "InfeasibleVelocity",
                 "InfeasibleRollPitchRates", "InfeasibleYawRates", "InfeasibleYawAcc")


def get_input_feasibility_result_name(result: int) -> str:
    """getInputFeasibilityResultName: the enumerator without its kInput prefix."""
    result = int(result)
    return _RESULT_NAMES[result] if 0 <= result < len(_RESULT_NAMES) else "Unknown!"


class InputConstraints:
    """The reference's InputConstraints (input_constraints.h): up to six optional limits, stored by magnitude.  Adding f_min
    while f_max exists raises f_max to at least it, and the mirror case.  gravity enters the thrust ||a + (0, 0, gravity)||
    and the default thrust limits; min_section_time_s is FeasibilityAnalytic::Settings' (stored by magnitude too)."""
    NAMES = ("f_min", "f_max", "v_max", "omega_xy_max", "omega_z_max", "omega_z_dot_max")
    GRAVITY = 9.81   # mav_msgs::kGravity upstream

    def __init__(self, min_section_time_s: float = 0.05, gravity: float = GRAVITY, **limits):
        self.constraints = {}
        self.min_section_time_s = abs(float(min_section_time_s))
        self.gravity = float(gravity)
        for name, value in limits.items():
            self.add_constraint(name, value)

    @classmethod
    def defaults(cls, **kw) -> "InputConstraints":
        c = cls(**kw)
        c.set_default_values()
        return c

    def add_constraint(self, name: str, value: float):
        if name not in self.NAMES:
            raise KeyError(name)
        value = abs(float(value))
        if name == "f_min" and "f_max" in self.constraints:
            self.constraints["f_max"] = max(value, self.constraints["f_max"])
        elif name == "f_max" and "f_min" in self.constraints:
            self.constraints["f_min"] = min(value, self.constraints["f_min"])
        self.constraints[name] = value

    def set_default_values(self):
        import math
        self.constraints.update(f_min=0.5 * self.gravity, f_max=1.5 * self.gravity, v_max=3.0, omega_xy_max=math.pi / 2.0,
                                omega_z_max=math.pi / 2.0, omega_z_dot_max=2.0 * math.pi)

    def has_constraint(self, name: str) -> bool:
        return name in self.constraints

    def get_constraint(self, name: str) -> Optional[float]:
        return self.constraints.get(name)

    def remove_constraint(self, name: str) -> bool:
        return self.constraints.pop(name, None) is not None

    def to_c(self) -> L.InputConstraintsC:
        c = L.InputConstraintsC(*[self.constraints.get(n, float("nan")) for n in self.NAMES], self.min_section_time_s, self.gravity)
        return c


def check_input_feasibility(ctx: "Context", coeffs, times, constraints: InputConstraints, times_layout: str = "aos",
                            want_segments: bool = True, want_bounds: bool = True):
    """Batched FeasibilityAnalytic::checkInputFeasibilityTrajectory: coeffs [B][K][D][N], times ([B][K] 'aos' / [K][B] 'soa')
    CUDA tensors -> (trajectory_result [B] int32, first_failing_segment [B] int32 (-1: none), segment_result [B][K] int32 or
    None, segment_bounds [B][K][6] or None: thrust min, thrust max, velocity max, whole-segment roll/pitch bound, |yaw rate|
    max, |yaw acceleration| max; NaN where not computed).  Result codes: InputFeasibilityResult."""
    import torch
    bsz, k, dim, n = coeffs.shape
    assert coeffs.is_cuda and coeffs.dtype == torch.float64 and coeffs.is_contiguous() and times.is_contiguous()
    dev = coeffs.device
    traj = torch.empty((bsz,), dtype=torch.int32, device=dev)
    first = torch.empty((bsz,), dtype=torch.int32, device=dev)
    seg = torch.empty((bsz, k), dtype=torch.int32, device=dev) if want_segments else None
    bounds = torch.empty((bsz, k, 6), dtype=torch.float64, device=dev) if want_bounds else None
    sb, sk = (k, 1) if times_layout == "aos" else (1, bsz)
    c = constraints.to_c()
    cur = ctx._enter()
    rc = ctx.lib.mtg_check_input_feasibility(ctx.handle, n, k, dim, bsz, ctypes.c_void_p(coeffs.data_ptr()),
                                             ctypes.c_void_p(times.data_ptr()), sb, sk, ctypes.byref(c),
                                             ctypes.c_void_p(traj.data_ptr()), ctypes.c_void_p(first.data_ptr()),
                                             ctypes.c_void_p(seg.data_ptr()) if seg is not None else None,
                                             ctypes.c_void_p(bounds.data_ptr()) if bounds is not None else None)
    ctx._leave(cur)
    _check(ctx.lib, rc, ctx.handle)
    return traj, first, seg, bounds


def check_input_feasibility_host(coeffs, times, constraints: InputConstraints, times_layout: str = "aos"):
    """The same check on numpy arrays through the library's host build of the same code (no context, no device): coeffs
    [B][K][D][N] or one trajectory [K][D][N]; returns numpy (trajectory_result, first_failing_segment, segment_result,
    segment_bounds), shaped as the device form's (without the batch axis for one trajectory)."""
    lib = L.load()
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    times = np.ascontiguousarray(times, dtype=np.float64)
    single = coeffs.ndim == 3
    if single:
        coeffs, times = coeffs[None], times[None]
    bsz, k, dim, n = coeffs.shape
    if times.size != bsz * k:
        raise MtgError(-1, "times must hold one value per segment")
    traj = np.empty((bsz,), dtype=np.int32)
    first = np.empty((bsz,), dtype=np.int32)
    seg = np.empty((bsz, k), dtype=np.int32)
    bounds = np.empty((bsz, k, 6), dtype=np.float64)
    sb, sk = (k, 1) if times_layout == "aos" else (1, bsz)
    c = constraints.to_c()
    rc = lib.mtg_check_input_feasibility_host(n, k, dim, bsz, coeffs.ctypes.data, times.ctypes.data, sb, sk, ctypes.byref(c),
                                              traj.ctypes.data, first.ctypes.data, seg.ctypes.data, bounds.ctypes.data)
    _check(lib, rc)
    if single:
        return traj[0], first[0], seg[0], bounds[0]
    return traj, first, seg, bounds


def check_input_feasibility_recursive(ctx: "Context", coeffs, times, constraints: InputConstraints, times_layout: str = "aos",
                                      want_segments: bool = True, want_bounds: bool = True, want_sections: bool = False):
    """Batched FeasibilityRecursive::checkInputFeasibilityTrajectory (Mueller's recursive test on single-axis extrema, the cheap
    and conservative checker): the arguments of check_input_feasibility -> (trajectory_result [B] int32, first_failing_segment
    [B] int32 (-1: none), segment_result [B][K] int32 or None, segment_bounds [B][K][6] or None: f_lower_bound, f_upper_bound,
    v_upper_bound and roll/pitch bound of the whole-segment section [0, T], |yaw rate| max, |yaw acceleration| max; NaN where
    not computed, segment_sections [B][K] int32 or None: the sections the walk examined).  constraints.min_section_time_s is
    FeasibilityRecursive::Settings' value.  Result codes: InputFeasibilityResult."""
    import torch
    bsz, k, dim, n = coeffs.shape
    assert coeffs.is_cuda and coeffs.dtype == torch.float64 and coeffs.is_contiguous() and times.is_contiguous()
    dev = coeffs.device
    traj = torch.empty((bsz,), dtype=torch.int32, device=dev)
    first = torch.empty((bsz,), dtype=torch.int32, device=dev)
    seg = torch.empty((bsz, k), dtype=torch.int32, device=dev) if want_segments else None
    bounds = torch.empty((bsz, k, 6), dtype=torch.float64, device=dev) if want_bounds else None
    sections = torch.empty((bsz, k), dtype=torch.int32, device=dev) if want_sections else None
    sb, sk = (k, 1) if times_layout == "aos" else (1, bsz)
    c = constraints.to_c()
    cur = ctx._enter()
    rc = ctx.lib.mtg_check_input_feasibility_recursive(
        ctx.handle, n, k, dim, bsz, ctypes.c_void_p(coeffs.data_ptr()), ctypes.c_void_p(times.data_ptr()), sb, sk, ctypes.byref(c),
        ctypes.c_void_p(traj.data_ptr()), ctypes.c_void_p(first.data_ptr()),
        ctypes.c_void_p(seg.data_ptr()) if seg is not None else None,
        ctypes.c_void_p(bounds.data_ptr()) if bounds is not None else None,
        ctypes.c_void_p(sections.data_ptr()) if sections is not None else None)
    ctx._leave(cur)
    _check(ctx.lib, rc, ctx.handle)
    return traj, first, seg, bounds, sections


def check_input_feasibility_recursive_host(coeffs, times, constraints: InputConstraints, times_layout: str = "aos"):
    """The same check on numpy arrays through the library's host build of the same code (no context, no device): coeffs
    [B][K][D][N] or one trajectory [K][D][N]; returns numpy (trajectory_result, first_failing_segment, segment_result,
    segment_bounds, segment_sections), shaped as the device form's (without the batch axis for one trajectory)."""
    lib = L.load()
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    times = np.ascontiguousarray(times, dtype=np.float64)
    single = coeffs.ndim == 3
    if single:
        coeffs, times = coeffs[None], times[None]
    bsz, k, dim, n = coeffs.shape
    if times.size != bsz * k:
        raise MtgError(-1, "times must hold one value per segment")
    traj = np.empty((bsz,), dtype=np.int32)
    first = np.empty((bsz,), dtype=np.int32)
    seg = np.empty((bsz, k), dtype=np.int32)
    bounds = np.empty((bsz, k, 6), dtype=np.float64)
    sections = np.empty((bsz, k), dtype=np.int32)
    sb, sk = (k, 1) if times_layout == "aos" else (1, bsz)
    c = constraints.to_c()
    rc = lib.mtg_check_input_feasibility_recursive_host(n, k, dim, bsz, coeffs.ctypes.data, times.ctypes.data, sb, sk,
                                                        ctypes.byref(c), traj.ctypes.data, first.ctypes.data, seg.ctypes.data,
                                                        bounds.ctypes.data, sections.ctypes.data)
    _check(lib, rc)
    if single:
        return traj[0], first[0], seg[0], bounds[0], sections[0]
    return traj, first, seg, bounds, sections


def half_planes(points, normals) -> np.ndarray:
    """HalfPlane(point, normal) for n planes: points [n][3], normals [n][3] (any length > 0) -> [n][4] rows (unit normal,
    offset = point . normal), the plane format of check_half_plane_feasibility.  A zero normal raises."""
    lib = L.load()
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3)
    if points.shape != normals.shape:
        raise MtgError(-1, "one point per normal")
    out = np.empty((points.shape[0], 4), dtype=np.float64)
    _check(lib, lib.mtg_half_planes_from_points_normals(points.shape[0], points.ctypes.data, normals.ctypes.data, out.ctypes.data))
    return out


def bounding_box_half_planes(center, size) -> np.ndarray:
    """HalfPlane::createBoundingBox(center, size) -> [6][4]: per axis the minimum face with +e, then the maximum face with -e."""
    lib = L.load()
    center = np.ascontiguousarray(center, dtype=np.float64).reshape(3)
    size = np.ascontiguousarray(size, dtype=np.float64).reshape(3)
    out = np.empty((6, 4), dtype=np.float64)
    _check(lib, lib.mtg_half_planes_bounding_box(center.ctypes.data, size.ctypes.data, out.ctypes.data))
    return out


class HalfPlaneFeasibilityResult(NamedTuple):
    """trajectory_feasible [B] int32 (1 / 0), first_failing_segment [B] int32 (-1: none), first_failing_plane [B] int32
    (-1: none), segment_clearance [B][K] or None, trajectory_clearance [B] or None (minimum signed distance to the planes)."""
    trajectory_feasible: object
    first_failing_segment: object
    first_failing_plane: object
    segment_clearance: object
    trajectory_clearance: object


def _plane_strides(shape, bsz: int, k: int):
    """[P][4]: one set for everything; [K][P][4]: one cell per segment; [B][K][P][4]: a corridor per trajectory."""
    if len(shape) not in (2, 3, 4) or shape[-1] != 4:
        raise MtgError(-1, "planes must be [P][4], [K][P][4] or [B][K][P][4]")
    p = int(shape[-2])
    if len(shape) >= 3 and shape[-3] != k or len(shape) == 4 and shape[0] != bsz:
        raise MtgError(-1, "planes: the segment / batch axes must match coeffs")
    return p, (4 * p * k if len(shape) == 4 else 0), (4 * p if len(shape) >= 3 else 0)


def check_half_plane_feasibility(ctx: "Context", coeffs, times, planes, times_layout: str = "aos",
                                 want_clearance: bool = True) -> HalfPlaneFeasibilityResult:
    """Batched FeasibilityBase::checkHalfPlaneFeasibility(Trajectory): coeffs [B][K][D][N], times ([B][K] 'aos' / [K][B] 'soa')
    and planes ([P][4], [K][P][4] or [B][K][P][4] rows of (unit normal, offset), see half_planes) as CUDA float64 tensors.
    A plane fails a segment iff n . p(t) - offset <= 0 at t = 0, T or a critical point of the projection."""
    import torch
    bsz, k, dim, n = coeffs.shape
    assert coeffs.is_cuda and coeffs.dtype == torch.float64 and coeffs.is_contiguous() and times.is_contiguous()
    assert planes.is_cuda and planes.dtype == torch.float64 and planes.is_contiguous()
    p, psb, psk = _plane_strides(tuple(planes.shape), bsz, k)
    dev = coeffs.device
    feas = torch.empty((bsz,), dtype=torch.int32, device=dev)
    fseg = torch.empty((bsz,), dtype=torch.int32, device=dev)
    fplane = torch.empty((bsz,), dtype=torch.int32, device=dev)
    seg_c = torch.empty((bsz, k), dtype=torch.float64, device=dev) if want_clearance else None
    traj_c = torch.empty((bsz,), dtype=torch.float64, device=dev) if want_clearance else None
    sb, sk = (k, 1) if times_layout == "aos" else (1, bsz)
    cur = ctx._enter()
    rc = ctx.lib.mtg_check_half_plane_feasibility(ctx.handle, n, k, dim, bsz, ctypes.c_void_p(coeffs.data_ptr()),
                                                  ctypes.c_void_p(times.data_ptr()), sb, sk, ctypes.c_void_p(planes.data_ptr()),
                                                  p, psb, psk, ctypes.c_void_p(feas.data_ptr()), ctypes.c_void_p(fseg.data_ptr()),
                                                  ctypes.c_void_p(fplane.data_ptr()),
                                                  ctypes.c_void_p(seg_c.data_ptr()) if seg_c is not None else None,
                                                  ctypes.c_void_p(traj_c.data_ptr()) if traj_c is not None else None)
    ctx._leave(cur)
    _check(ctx.lib, rc, ctx.handle)
    return HalfPlaneFeasibilityResult(feas, fseg, fplane, seg_c, traj_c)


def check_half_plane_feasibility_host(coeffs, times, planes, times_layout: str = "aos") -> HalfPlaneFeasibilityResult:
    """The same check on numpy arrays through the library's host build of the same code (no context, no device): coeffs
    [B][K][D][N] or one trajectory [K][D][N] (then planes [P][4] or [K][P][4], results without the batch axis).  Normals
    that are not of unit length raise."""
    lib = L.load()
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    times = np.ascontiguousarray(times, dtype=np.float64)
    planes = np.ascontiguousarray(planes, dtype=np.float64)
    single = coeffs.ndim == 3
    if single:
        coeffs, times = coeffs[None], times[None]
    bsz, k, dim, n = coeffs.shape
    if times.size != bsz * k:
        raise MtgError(-1, "times must hold one value per segment")
    p, psb, psk = _plane_strides(planes.shape, bsz, k)
    feas = np.empty((bsz,), dtype=np.int32)
    fseg = np.empty((bsz,), dtype=np.int32)
    fplane = np.empty((bsz,), dtype=np.int32)
    seg_c = np.empty((bsz, k), dtype=np.float64)
    traj_c = np.empty((bsz,), dtype=np.float64)
    sb, sk = (k, 1) if times_layout == "aos" else (1, bsz)
    rc = lib.mtg_check_half_plane_feasibility_host(n, k, dim, bsz, coeffs.ctypes.data, times.ctypes.data, sb, sk, planes.ctypes.data,
                                                   p, psb, psk, feas.ctypes.data, fseg.ctypes.data, fplane.ctypes.data,
                                                   seg_c.ctypes.data, traj_c.ctypes.data)
    _check(lib, rc)
    res = HalfPlaneFeasibilityResult(feas, fseg, fplane, seg_c, traj_c)
    return HalfPlaneFeasibilityResult(*[a[0] for a in res]) if single else res


def sphere_obstacles(centers, radii) -> np.ndarray:
    """centers [M][3] with radii [M] (or a scalar) -> [M][4] rows (cx, cy, cz, r), the obstacle format of
    check_obstacle_clearance; centers [B][M][3] with radii [M], [B][M] or a scalar -> [B][M][4], a set per trajectory.
    A radius that is negative or not finite raises."""
    centers = np.asarray(centers, dtype=np.float64)
    if centers.ndim not in (2, 3) or centers.shape[-1] != 3:
        raise MtgError(-1, "centers must be [M][3] or [B][M][3]")
    radii = np.broadcast_to(np.asarray(radii, dtype=np.float64), centers.shape[:-1])
    if not (np.isfinite(radii) & (radii >= 0.0)).all():
        raise MtgError(-1, "radii must be >= 0 and finite")
    return np.ascontiguousarray(np.concatenate([centers, radii[..., None]], axis=-1))


class ObstacleClearanceResult(NamedTuple):
    """trajectory_feasible [B] int32 (1 / 0), first_failing_segment [B] int32 (-1: none), first_failing_obstacle [B] int32
    (-1: none), segment_clearance [B][K], segment_nearest_obstacle [B][K] int32, segment_closest_time [B][K],
    trajectory_clearance [B] (minimum of ||p(t) - c|| - r - inflation; a NaN wins); the last four None if not asked for."""
    trajectory_feasible: object
    first_failing_segment: object
    first_failing_obstacle: object
    segment_clearance: object
    segment_nearest_obstacle: object
    segment_closest_time: object
    trajectory_clearance: object


def _obstacle_stride(shape, bsz: int):
    """[M][4]: one set for every trajectory; [B][M][4]: a set per trajectory."""
    if len(shape) not in (2, 3) or shape[-1] != 4:
        raise MtgError(-1, "obstacles must be [M][4] or [B][M][4]")
    m = int(shape[-2])
    if len(shape) == 3 and shape[0] != bsz:
        raise MtgError(-1, "obstacles: the batch axis must match coeffs")
    return m, (4 * m if len(shape) == 3 else 0)


def check_obstacle_clearance(ctx: "Context", coeffs, times, obstacles, inflation: float = 0.0, times_layout: str = "aos",
                             want_clearance: bool = True) -> ObstacleClearanceResult:
    """Batched clearance of solved trajectories from a set of spheres: coeffs [B][K][D][N] (D = 3 or 4), times ([B][K] 'aos' /
    [K][B] 'soa') and obstacles ([M][4] or [B][M][4] rows of (cx, cy, cz, r), see sphere_obstacles) as CUDA float64 tensors.
    An obstacle fails a segment iff not ||p(t) - c|| - r - inflation > 0 at t = 0, T or a critical point of the distance."""
    import torch
    bsz, k, dim, n = coeffs.shape
    assert coeffs.is_cuda and coeffs.dtype == torch.float64 and coeffs.is_contiguous() and times.is_contiguous()
    assert obstacles.is_cuda and obstacles.dtype == torch.float64 and obstacles.is_contiguous()
    m, osb = _obstacle_stride(tuple(obstacles.shape), bsz)
    dev = coeffs.device
    feas = torch.empty((bsz,), dtype=torch.int32, device=dev)
    fseg = torch.empty((bsz,), dtype=torch.int32, device=dev)
    fobs = torch.empty((bsz,), dtype=torch.int32, device=dev)
    seg_c = torch.empty((bsz, k), dtype=torch.float64, device=dev) if want_clearance else None
    seg_o = torch.empty((bsz, k), dtype=torch.int32, device=dev) if want_clearance else None
    seg_t = torch.empty((bsz, k), dtype=torch.float64, device=dev) if want_clearance else None
    traj_c = torch.empty((bsz,), dtype=torch.float64, device=dev) if want_clearance else None
    sb, sk = (k, 1) if times_layout == "aos" else (1, bsz)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    cur = ctx._enter()
    rc = ctx.lib.mtg_check_obstacle_clearance(ctx.handle, n, k, dim, bsz, ptr(coeffs), ptr(times), sb, sk, ptr(obstacles), m, osb,
                                              float(inflation), ptr(feas), ptr(fseg), ptr(fobs), ptr(seg_c), ptr(seg_o), ptr(seg_t),
                                              ptr(traj_c))
    ctx._leave(cur)
    _check(ctx.lib, rc, ctx.handle)
    return ObstacleClearanceResult(feas, fseg, fobs, seg_c, seg_o, seg_t, traj_c)


def check_obstacle_clearance_host(coeffs, times, obstacles, inflation: float = 0.0,
                                  times_layout: str = "aos") -> ObstacleClearanceResult:
    """The same check on numpy arrays through the library's host build of the same code (no context, no device): coeffs
    [B][K][D][N] or one trajectory [K][D][N] (then obstacles [M][4], results without the batch axis).  A radius that is
    negative or not finite raises."""
    lib = L.load()
    coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
    times = np.ascontiguousarray(times, dtype=np.float64)
    obstacles = np.ascontiguousarray(obstacles, dtype=np.float64)
    single = coeffs.ndim == 3
    if single:
        coeffs, times = coeffs[None], times[None]
    bsz, k, dim, n = coeffs.shape
    if times.size != bsz * k:
        raise MtgError(-1, "times must hold one value per segment")
    m, osb = _obstacle_stride(obstacles.shape, bsz)
    feas = np.empty((bsz,), dtype=np.int32)
    fseg = np.empty((bsz,), dtype=np.int32)
    fobs = np.empty((bsz,), dtype=np.int32)
    seg_c = np.empty((bsz, k), dtype=np.float64)
    seg_o = np.empty((bsz, k), dtype=np.int32)
    seg_t = np.empty((bsz, k), dtype=np.float64)
    traj_c = np.empty((bsz,), dtype=np.float64)
    sb, sk = (k, 1) if times_layout == "aos" else (1, bsz)
    rc = lib.mtg_check_obstacle_clearance_host(n, k, dim, bsz, coeffs.ctypes.data, times.ctypes.data, sb, sk, obstacles.ctypes.data,
                                               m, osb, float(inflation), feas.ctypes.data, fseg.ctypes.data, fobs.ctypes.data,
                                               seg_c.ctypes.data, seg_o.ctypes.data, seg_t.ctypes.data, traj_c.ctypes.data)
    _check(lib, rc)
    res = ObstacleClearanceResult(feas, fseg, fobs, seg_c, seg_o, seg_t, traj_c)
    return ObstacleClearanceResult(*[a[0] for a in res]) if single else res


class Plan:
    def __init__(self, ctx: Context, n_coeffs: int, dimension: int, n_segments: int,
                 derivative_to_optimize: Optional[int], fixed_mask: Sequence[int]):
        self.ctx = ctx
        self.lib = ctx.lib
        self.N, self.D, self.K = int(n_coeffs), int(dimension), int(n_segments)
        self.deriv = self.N // 2 - 1 if derivative_to_optimize is None else int(derivative_to_optimize)
        if len(fixed_mask) != self.K + 1:
            raise MtgError(-1, "fixed_mask must have n_segments + 1 entries")
        self.fixed_mask = [int(m) for m in fixed_mask]
        arr = (ctypes.c_uint32 * (self.K + 1))(*self.fixed_mask)
        desc = L.PlanDesc(self.N, self.D, self.K, self.deriv, arr)
        h = ctypes.c_void_p()
        _check(self.lib, self.lib.mtg_plan_create(ctx.handle, ctypes.byref(desc), ctypes.byref(h)), ctx.handle)
        self.handle = h
        ctx._plans.add(self)
        info = L.PlanInfo()
        _check(self.lib, self.lib.mtg_plan_get_info(h, ctypes.byref(info)))
        self.n_all, self.n_fixed, self.n_free = info.n_all, info.n_fixed, info.n_free
        self.kernel_variant = info.kernel_variant
        self.bytes_per_trajectory = info.algorithmic_bytes_per_trajectory
        # structural rank deficiency of the free system (0: regular; > 0: every solve flags every trajectory singular and
        # basic_solution=True gives the reference's basic solution, LIN:365-378)
        self.rank_deficiency = self.lib.mtg_plan_rank_deficiency(h)

    def layout(self, batch: int, kind: str) -> L.Layout:
        lay = L.Layout()
        if kind == "aos":
            self.lib.mtg_layout_aos(self.handle, batch, ctypes.byref(lay))
        elif kind == "soa":
            self.lib.mtg_layout_soa(self.handle, batch, ctypes.byref(lay))
        elif kind == "soa16":     # SoA, row stride padded to a multiple of 16 trajectories (mtg_layout_soa_padded)
            self.lib.mtg_layout_soa_padded(self.handle, batch, ctypes.byref(lay))
        else:
            raise ValueError(kind)
        return lay

    @staticmethod
    def _ptr(t):
        return ctypes.c_void_p(0) if t is None else ctypes.c_void_p(t.data_ptr())

    def generate_waypoints(self, batch: int, seed: int = 0, layout: str = "soa", box: float = 10.0, v_max: float = 3.0,
                           a_max: float = 5.0, yaw_dim: bool = False):
        """Random-waypoint inputs of this plan's structure generated by the library's own kernel (C ABI:
        mtg_generate_waypoints; the torch generator of workload.py has the same semantics).  Returns (times, d_fixed) float64
        CUDA tensors in `layout`.  Asynchronous on the library's stream (ordered against torch's current stream)."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        if layout == "soa":
            t = torch.empty((self.K, batch), dtype=torch.float64, device=dev)
            f = torch.empty((self.D, self.n_fixed, batch), dtype=torch.float64, device=dev)
        else:
            t = torch.empty((batch, self.K), dtype=torch.float64, device=dev)
            f = torch.empty((batch, self.D, self.n_fixed), dtype=torch.float64, device=dev)
        lay = self.layout(batch, layout)
        cur = self.ctx._enter()
        rc = self.lib.mtg_generate_waypoints(self.handle, batch, ctypes.byref(lay), int(seed) & (2**64 - 1), float(box),
                                             float(v_max), float(a_max), 1 if yaw_dim else 0, self._ptr(t), self._ptr(f))
        self.ctx._leave(cur)
        _check(self.lib, rc, self.ctx.handle)
        return t, f

    def solve(self, times, d_fixed, layout: str = "aos", want_free: bool = False, want_cost: bool = False,
              coeffs=None, d_free=None, cost=None, generic: bool = False, dims: str = "auto", ordered: bool = True,
              traj_status=None, basic_solution: bool = False, batch: Optional[int] = None, refine: bool = False):
        """times / d_fixed: float64 CUDA tensors in `layout` ('aos': [B][K], [B][D][n_fixed];
        'soa': [K][B], [D][n_fixed][B]).  Asynchronous; returns (coeffs [B][K][D][N], d_free, cost).
        dims: launch form -- 'auto', 'fused', 'split' (one dimension group per workgroup) or 'dimlane' (all dimensions of
        a trajectory in one wavefront; canonical SoA or AoS inputs, coefficient output only -- falls back to 'auto' where
        not eligible).
        traj_status: optional int32 CUDA tensor [B] that receives the per-trajectory status bits (1 bad time, 2 singular).
        basic_solution: the reference's behaviour on rank-deficient free systems (MTG_FLAG_BASIC_SOLUTION: flagged trajectories
        get the basic solution of a pivoted QR on the host; the call is then synchronous).
        refine: MTG_FLAG_REFINE -- one step of iterative refinement with the residual in double-double (conditioning-limited
        problems: N = 12, d < N/2 - 1); about five plain solves.
        ordered=False skips the automatic ordering against torch's current stream (the caller forks / joins the
        context's stream itself -- MixedBatchSolver runs independent buckets concurrently that way); output tensors
        must then be passed in, allocated by the caller before the fork."""
        import torch
        if layout == "soa16":
            # times [K][Bs], d_fixed [D][n_fixed][Bs] with Bs = batch rounded up to a multiple of 16: the batch size itself
            # cannot be read off the tensors
            assert batch is not None and times.shape[1] == ((batch + 15) & ~15), "layout 'soa16' needs batch= and padded tensors"
        else:
            batch = times.shape[0] if layout == "aos" else times.shape[1]
        assert times.dtype == torch.float64 and times.is_cuda and times.is_contiguous()
        assert d_fixed.dtype == torch.float64 and d_fixed.is_cuda and d_fixed.is_contiguous()
        dev = times.device
        if coeffs is None:
            coeffs = torch.empty((batch, self.K, self.D, self.N), dtype=torch.float64, device=dev)
        if want_free and d_free is None:
            shape = (batch, self.D, self.n_free) if layout == "aos" else (self.D, self.n_free, batch if layout == "soa" else (batch + 15) & ~15)
            d_free = torch.empty(shape, dtype=torch.float64, device=dev)
        if want_cost and cost is None:
            cost = torch.empty((batch,), dtype=torch.float64, device=dev)
        lay = self.layout(batch, layout)
        flags = L.FLAG_GENERIC_KERNEL if generic else 0
        flags |= {"auto": 0, "fused": L.FLAG_FUSED_DIMS, "split": L.FLAG_SPLIT_DIMS, "dimlane": L.FLAG_DIMLANE, "coop": L.FLAG_COOPERATIVE}[dims]
        if basic_solution:
            flags |= L.FLAG_BASIC_SOLUTION
        if refine:
            flags |= L.FLAG_REFINE
        if traj_status is not None:
            assert traj_status.dtype == torch.int32 and traj_status.is_cuda and traj_status.numel() >= batch
        cur = self.ctx._enter() if ordered else None
        rc = self.lib.mtg_solve_linear_status(self.handle, batch, ctypes.byref(lay), self._ptr(times),
                                              self._ptr(d_fixed), self._ptr(coeffs), self._ptr(d_free), self._ptr(cost),
                                              self._ptr(traj_status), flags)
        if ordered:
            self.ctx._leave(cur)
        _check(self.lib, rc, self.ctx.handle)
        return coeffs, d_free, cost

    def solve_sequence(self, sets, layout: str = "soa", dims: str = "auto", one_launch_per_batch: bool = False,
                       start_event=None, stop_event=None, ordered: bool = True, basic_solution: bool = False):
        """A queue of INDEPENDENT batches of equal size (mtg_solve_linear_sequence[_events]): `sets` = sequence of
        (times, d_fixed, coeffs) CUDA tensors in `layout`, coeffs [B][K][D][N] allocated by the caller.  Plans with a
        slab-output kernel run the whole queue as ONE persistent launch (workgroups walk the tiles of all batches);
        one_launch_per_batch=True keeps one launch per batch.  start_event / stop_event: torch.cuda.Event objects that
        have been recorded once (their hipEvent_t exists), recorded by the library around the queue."""
        import torch
        n = len(sets)
        if n == 0:
            return
        batch = sets[0][2].shape[0]
        for (t, f, co) in sets:
            assert t.dtype == torch.float64 and t.is_cuda and t.is_contiguous()
            assert f.dtype == torch.float64 and f.is_cuda and f.is_contiguous()
            assert co.dtype == torch.float64 and co.is_cuda and co.is_contiguous() and co.shape[0] == batch
        arr = [(ctypes.c_void_p * n)(*[x[j].data_ptr() for x in sets]) for j in range(3)]
        lay = self.layout(batch, layout)
        flags = {"auto": 0, "fused": L.FLAG_FUSED_DIMS, "split": L.FLAG_SPLIT_DIMS, "dimlane": L.FLAG_DIMLANE, "coop": L.FLAG_COOPERATIVE}[dims]
        if one_launch_per_batch:
            flags |= L.FLAG_SEQUENCE_ONE_LAUNCH_PER_BATCH
        if basic_solution:   # a structurally rank-deficient plan runs the queue on its shadow (asynchronous; LIN:365-378)
            flags |= L.FLAG_BASIC_SOLUTION
        ev = [ctypes.c_void_p(e.cuda_event) if e is not None else None for e in (start_event, stop_event)]
        cur = self.ctx._enter() if ordered else None
        rc = self.lib.mtg_solve_linear_sequence_events(self.handle, n, batch, ctypes.byref(lay), arr[0], arr[1], arr[2],
                                                       flags, ev[0], ev[1])
        if ordered:
            self.ctx._leave(cur)
        _check(self.lib, rc, self.ctx.handle)

    def solve_cost_only(self, times, d_fixed, layout: str = "aos", cost=None):
        """computeCost() of the optimum for every trajectory without materialising the segments
        (MTG_FLAG_COST_ONLY): what the time optimisers' objective callbacks need.  Returns cost [B]."""
        import torch
        batch = times.shape[0] if layout == "aos" else times.shape[1]
        if cost is None:
            cost = torch.empty((batch,), dtype=torch.float64, device=times.device)
        lay = self.layout(batch, layout)
        cur = self.ctx._enter()
        rc = self.lib.mtg_solve_linear(self.handle, batch, ctypes.byref(lay), self._ptr(times), self._ptr(d_fixed),
                                       None, None, self._ptr(cost), L.FLAG_COST_ONLY)
        self.ctx._leave(cur)
        _check(self.lib, rc, self.ctx.handle)
        return cost

    def update_from_free(self, times, d_fixed, d_free, layout: str = "aos", want_cost: bool = False):
        """setFreeConstraints() path: coefficients from given free constraints, no solve."""
        import torch
        batch = times.shape[0] if layout == "aos" else times.shape[1]
        dev = times.device
        coeffs = torch.empty((batch, self.K, self.D, self.N), dtype=torch.float64, device=dev)
        cost = torch.empty((batch,), dtype=torch.float64, device=dev) if want_cost else None
        lay = self.layout(batch, layout)
        cur = self.ctx._enter()
        rc = self.lib.mtg_update_segments_from_free(self.handle, batch, ctypes.byref(lay), self._ptr(times),
                                                    self._ptr(d_fixed), self._ptr(d_free), self._ptr(coeffs),
                                                    self._ptr(cost), 0)
        self.ctx._leave(cur)
        _check(self.lib, rc, self.ctx.handle)
        return coeffs, cost

    def solve_host(self, times: np.ndarray, d_fixed: np.ndarray, want_free=True, want_cost=True, generic=False,
                   coeffs: Optional[np.ndarray] = None, host_backend: bool = False, basic_solution: bool = False):
        """Host-buffer convenience (AoS numpy in/out, staged through the device by the library).  Pass page-locked
        arrays (e.g. pinned torch tensors viewed as numpy, also for `coeffs`) to have them DMA'd directly."""
        times = np.ascontiguousarray(times, dtype=np.float64)
        d_fixed = np.ascontiguousarray(d_fixed, dtype=np.float64)
        batch = times.shape[0]
        if coeffs is None:
            coeffs = np.empty((batch, self.K, self.D, self.N))
        assert coeffs.dtype == np.float64 and coeffs.flags.c_contiguous and coeffs.size == batch * self.K * self.D * self.N
        d_free = np.empty((batch, self.D, self.n_free)) if want_free else None
        cost = np.empty((batch,)) if want_cost else None
        lay = self.layout(batch, "aos")
        p = lambda a: ctypes.c_void_p(0) if a is None else ctypes.c_void_p(a.ctypes.data)
        flags = L.FLAG_HOST_POINTERS | (L.FLAG_GENERIC_KERNEL if generic else 0)
        if host_backend:   # batch <= 64: the lane code's host build on this thread (latency path), no GPU involved
            flags |= L.FLAG_HOST_BACKEND
        if basic_solution:  # rank-deficient trajectories get the reference's basic solution (LIN:365-378)
            flags |= L.FLAG_BASIC_SOLUTION
        rc = self.lib.mtg_solve_linear(self.handle, batch, ctypes.byref(lay), p(times), p(d_fixed), p(coeffs),
                                       p(d_free), p(cost), flags)
        _check(self.lib, rc, self.ctx.handle)
        return coeffs, d_free, cost

    LAUNCH_FORMS = {0: "generic", 1: "fused", 2: "split", 3: "rolled", 4: "slab", 5: "dimlane", 6: "dimlane_rt", 7: "coop"}

    def launch_form(self, batch: int, layout: str = "soa", dims: str = "auto", extra_outputs: bool = False) -> str:
        """Kernel form a coefficient-only device-pointer solve of `batch` trajectories takes (mtg_plan_launch_form);
        extra_outputs: of a solve that also returns the cost / d_free."""
        lay = self.layout(batch, layout)
        flags = {"auto": 0, "fused": L.FLAG_FUSED_DIMS, "split": L.FLAG_SPLIT_DIMS, "dimlane": L.FLAG_DIMLANE, "coop": L.FLAG_COOPERATIVE}[dims]
        if extra_outputs:
            flags |= L.FLAG_QUERY_EXTRA_OUTPUTS
        rc = self.lib.mtg_plan_launch_form(self.handle, batch, ctypes.byref(lay), flags)
        if rc < 0:
            _check(self.lib, rc, self.ctx.handle)
        return self.LAUNCH_FORMS[rc]

    def time_last_solve(self, iters: int = 100) -> float:
        """Mean device duration (us) of the last solve launch, hipEvents on the context stream."""
        out = ctypes.c_double(0)
        _check(self.lib, self.lib.mtg_time_last_solve(self.handle, iters, ctypes.byref(out)), self.ctx.handle)
        return out.value

    def close(self):
        if getattr(self, "handle", None):
            if getattr(self.ctx, "handle", None):   # a plan outliving its context is already gone on the C side
                self.lib.mtg_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# numpy mirror of mtg_multi_item (include/mtg_hip.h): a request of hundreds of items is put together by concatenating
# pre-packed arrays instead of filling ctypes structures item by item (240 items: ~1 ms of Python against ~20 us)
MULTI_ITEM_DTYPE = np.dtype([("plan", np.uint64), ("batch", np.int64), ("layout", np.int64, (8,)), ("times", np.uint64),
                             ("d_fixed", np.uint64), ("coeffs", np.uint64), ("d_free", np.uint64), ("cost", np.uint64)])
assert MULTI_ITEM_DTYPE.itemsize == ctypes.sizeof(L.MultiItem)


def pack_multi_items(items: Sequence[dict]) -> np.ndarray:
    """items: dicts with plan, times, d_fixed, coeffs (CUDA tensors; layout 'aos' | 'soa') -> packed mtg_multi_item array.
    The tensors must outlive every request created from the array."""
    out = np.zeros(len(items), dtype=MULTI_ITEM_DTYPE)
    for i, it in enumerate(items):
        plan: Plan = it["plan"]
        layout = it.get("layout", "aos")
        t = it["times"]
        batch = t.shape[0] if layout == "aos" else t.shape[1]
        lay = plan.layout(batch, layout)
        out[i]["plan"] = plan.handle.value
        out[i]["batch"] = batch
        out[i]["layout"] = [lay.times_stride_b, lay.times_stride_k, lay.fixed_stride_b, lay.fixed_stride_d, lay.fixed_stride_c,
                            lay.free_stride_b, lay.free_stride_d, lay.free_stride_c]
        out[i]["times"], out[i]["d_fixed"], out[i]["coeffs"] = t.data_ptr(), it["d_fixed"].data_ptr(), it["coeffs"].data_ptr()
    return out


class PackedMultiSolve:
    """A mixed request created from a packed mtg_multi_item array (pack_multi_items / np.concatenate of such arrays):
    coefficient output only.  create_us = host time of the mtg_multi_create call itself."""

    def __init__(self, ctx: Context, packed: np.ndarray, keep=None):
        import time
        assert packed.dtype == MULTI_ITEM_DTYPE and packed.flags.c_contiguous
        self.ctx, self.lib, self.keep = ctx, ctx.lib, keep
        h = ctypes.c_void_p()
        t0 = time.perf_counter()
        rc = self.lib.mtg_multi_create(ctx.handle, len(packed), packed.ctypes.data_as(ctypes.POINTER(L.MultiItem)), 0, ctypes.byref(h))
        self.create_us = (time.perf_counter() - t0) * 1e6
        _check(self.lib, rc, ctx.handle)
        self.handle = h
        self.launch_count = self.lib.mtg_multi_launch_count(h)
        ctx._plans.add(self)

    def solve(self, ordered: bool = True):
        """Enqueue the request on the context's stream (asynchronous).  ordered: the library's stream waits for torch's current
        stream before the launch and torch's current stream for the launch afterwards, as every other wrapper does
        (ordered=False: the caller orders the streams itself -- bench.py records its events on ctx.stream and syncs)."""
        cur = self.ctx._enter() if ordered else None
        try:
            rc = self.lib.mtg_multi_solve(self.handle)
        finally:
            if ordered:
                self.ctx._leave(cur)
        _check(self.lib, rc, self.ctx.handle)

    def close(self):
        if getattr(self, "handle", None):
            if getattr(self.ctx, "handle", None):
                self.lib.mtg_multi_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiSolve:
    """A mixed request (mtg_multi_*): several (plan, batch) items created once, solved as often as wanted with new
    values in the same device tensors.  Items that share N, D, the constraint pattern and the derivative run as ONE
    kernel launch.  items: dicts with plan, times, d_fixed (CUDA tensors), optional layout ('aos' | 'soa'), coeffs,
    d_free, cost tensors (coeffs allocated here when missing; cost / d_free only when want_cost / want_free)."""

    def __init__(self, ctx: Context, items: Sequence[dict], want_cost: bool = False, want_free: bool = False,
                 dims: str = "auto", basic_solution: bool = False):
        import torch
        self.ctx, self.lib = ctx, ctx.lib
        self.items = []
        arr = (L.MultiItem * len(items))()
        for i, it in enumerate(items):
            plan: Plan = it["plan"]
            assert plan.ctx is ctx
            layout = it.get("layout", "aos")
            t, f = it["times"], it["d_fixed"]
            batch = t.shape[0] if layout == "aos" else t.shape[1]
            co = it.get("coeffs")
            if co is None:
                co = torch.empty((batch, plan.K, plan.D, plan.N), dtype=torch.float64, device=t.device)
            cost = it.get("cost")
            if cost is None and want_cost:
                cost = torch.empty((batch,), dtype=torch.float64, device=t.device)
            fr = it.get("d_free")
            if fr is None and want_free:
                shape = (batch, plan.D, plan.n_free) if layout == "aos" else (plan.D, plan.n_free, batch)
                fr = torch.empty(shape, dtype=torch.float64, device=t.device)
            arr[i].plan = plan.handle
            arr[i].batch = batch
            arr[i].layout = plan.layout(batch, layout)
            arr[i].times, arr[i].d_fixed, arr[i].coeffs = t.data_ptr(), f.data_ptr(), co.data_ptr()
            arr[i].d_free = fr.data_ptr() if fr is not None else None
            arr[i].cost = cost.data_ptr() if cost is not None else None
            self.items.append(dict(plan=plan, times=t, d_fixed=f, coeffs=co, d_free=fr, cost=cost, layout=layout))
        h = ctypes.c_void_p()
        flags = {"auto": 0, "fused": L.FLAG_FUSED_DIMS, "split": L.FLAG_SPLIT_DIMS,
                 "concurrent": L.FLAG_CONCURRENT_ITEMS}[dims]   # concurrent: one launch per item on the context's side streams
        if basic_solution:   # items of structurally rank-deficient plans run on the plan's shadow (MTG_FLAG_BASIC_SOLUTION)
            flags |= L.FLAG_BASIC_SOLUTION
        _check(self.lib, self.lib.mtg_multi_create(ctx.handle, len(items), arr, flags, ctypes.byref(h)), ctx.handle)
        self.handle = h
        self.launch_count = self.lib.mtg_multi_launch_count(h)
        ctx._plans.add(self)   # closed with the context

    def solve(self, ordered: bool = True):
        """Enqueue the whole request (asynchronous).  Returns [(coeffs, d_free, cost)] in item order."""
        cur = self.ctx._enter() if ordered else None
        rc = self.lib.mtg_multi_solve(self.handle)
        if ordered:
            self.ctx._leave(cur)
        _check(self.lib, rc, self.ctx.handle)
        return [(it["coeffs"], it["d_free"], it["cost"]) for it in self.items]

    def close(self):
        if getattr(self, "handle", None):
            if getattr(self.ctx, "handle", None):
                self.lib.mtg_multi_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def solve_linear_batch(n_coeffs, derivative, fixed_mask, times: np.ndarray, d_fixed: np.ndarray, device: int = 0,
                       generic: bool = False):
    """One-shot host convenience: numpy AoS in -> (coeffs, d_free, cost) numpy out, via the HIP path."""
    ctx = Context(device)
    dim = d_fixed.shape[1]
    plan = Plan(ctx, n_coeffs, dim, times.shape[1], derivative, fixed_mask)
    out = plan.solve_host(times, d_fixed, generic=generic)
    ctx.sync()
    plan.close()
    ctx.close()
    return out
