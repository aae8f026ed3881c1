"""The batched per-segment calls: everything that takes a solved batch `coeffs [B][K][D][N]` with strided `times` -- sampling,
extrema, time scaling, the input-feasibility, half-plane, obstacle, separation and distance-field checks, the distance-field
collision cost and the time objective's soft cost -- in the device
form (CUDA tensors, a Context) and the host form (numpy, the library's host build of the same lane code).

This is the Python half of the frame the C++ side has in csrc/mtg_segment_lane.h / mtg_segment_kernel.h: _SegmentBatch validates
the inputs, allocates the outputs, turns the arguments into addresses, orders the streams and checks the status, once, for both
forms.  A check writes its docstring, its own argument rules, the list of its outputs and one `call`.
"""
from __future__ import annotations

import ctypes
import enum
from typing import TYPE_CHECKING, NamedTuple, Optional, Sequence

import numpy as np

from . import _lib as L
from .core import MtgError, _check

if TYPE_CHECKING:
    from .time_objective_search import TimeObjectiveParams


def _bad(what: str):
    raise MtgError(-1, what)


def _address(a: np.ndarray) -> int:
    """Where a numpy array's data is.  ctypes' from_buffer costs a quarter of ndarray.ctypes (0.3 us against 1 us per array, which
    is most of what a host form spends outside the library), but takes writable, non-empty arrays only."""
    if a.flags.writeable and a.size:
        return ctypes.addressof(ctypes.c_char.from_buffer(a))
    return a.ctypes.data


class _SegmentBatch:
    """One (coeffs, times, times_layout) of a per-segment call: the device form (ctx, torch) or the host form (ctx None, numpy).
    B, K, D, N: the shape of coeffs; f64, i32: the form's dtypes; single: the call was for one trajectory [K][D][N]."""
    __slots__ = ("ctx", "coeffs", "times", "B", "K", "D", "N", "single", "f64", "i32", "_strides", "_new", "_kind")

    def _shape(self, n_times: int, times_layout: str):
        """B, K, D, N and the strides of `times`; what both forms demand of them."""
        bsz, k, self.D, self.N = self.coeffs.shape
        self.B, self.K = bsz, k
        if n_times != bsz * k:
            _bad("times must hold one value per segment (%d x %d)" % (bsz, k))
        if times_layout == "aos":
            self._strides, other = (k, 1), (k, bsz)
        elif times_layout == "soa":
            self._strides, other = (1, bsz), (bsz, k)
        else:
            _bad("times_layout must be 'aos' or 'soa'")
        # (with one row or one column both layouts are the same memory)
        if bsz != k and bsz > 1 and k > 1 and tuple(self.times.shape) == other:
            _bad("times has the shape of the other layout, not of %r" % times_layout)

    @classmethod
    def device(cls, ctx, coeffs, times, times_layout: str):
        """coeffs [B][K][D][N] and times: float64 contiguous CUDA tensors on the context's device."""
        import torch
        self = cls()
        self.ctx, self.coeffs, self.times, self.single, self._new = ctx, coeffs, times, False, coeffs.new_empty
        self.f64, self.i32, self._kind = f64, _, _ = torch.float64, torch.int32, torch.Tensor
        if coeffs.dtype is not f64 or times.dtype is not f64:
            _bad("coeffs and times must be float64 tensors")
        if coeffs.dim() != 4:
            _bad("coeffs must be [B][K][D][N]")
        if not (coeffs.is_contiguous() and times.is_contiguous()):
            _bad("coeffs and times must be contiguous")
        self._shape(times.numel(), times_layout)
        if not coeffs.is_cuda:
            _bad("coeffs is not a CUDA tensor")
        if coeffs.get_device() != ctx.device:
            _bad("coeffs must be on the context's device %d" % ctx.device)
        if times.get_device() != ctx.device:
            _bad("times must be on the device of coeffs")
        return self

    @classmethod
    def host(cls, coeffs, times, times_layout: str):
        """coeffs [B][K][D][N] or one trajectory [K][D][N] (the results then come without the batch axis) and times: array-likes."""
        self = cls()
        coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
        self.single = coeffs.ndim == 3
        if coeffs.ndim not in (3, 4):
            _bad("coeffs must be [B][K][D][N] or [K][D][N]")
        self.ctx, self.coeffs, self.times = None, coeffs[None] if self.single else coeffs, np.ascontiguousarray(times, dtype=np.float64)
        self.f64, self.i32, self._new = np.float64, np.int32, np.empty
        self._shape(self.times.size, times_layout)
        return self

    def empty(self, shape, dtype, want: bool = True):
        """An uninitialised output next to coeffs (dtype: self.f64 / self.i32), or None if it is not wanted."""
        return self._new(shape, dtype=dtype) if want else None

    def extra(self, x, what: str, dtype: str = "float64"):
        """A further input of one dtype (planes, obstacles, a workspace: float64; a voxel grid: float32): validated on the device
        form, converted on the host form."""
        if self.ctx is None:
            return np.ascontiguousarray(x, dtype=dtype)
        import torch
        if x.dtype is not getattr(torch, dtype):
            _bad("%s must be a %s tensor" % (what, dtype))
        if not x.is_contiguous():
            _bad("%s must be contiguous" % what)
        if x.device != self.coeffs.device:
            _bad("%s must be on the device of coeffs" % what)
        return x

    def call(self, name: str, *tail):
        """lib.<name>(ctx, N, K, D, B, coeffs, times, sb, sk, *tail) between _enter / _leave on the device form,
        lib.<name>_host(N, K, D, B, ...) on the host form; tensors, arrays and None in `tail` become addresses."""
        ctx = self.ctx
        if ctx is None:
            lib = L.load()
            args = [_address(a) if isinstance(a, np.ndarray) else a for a in tail]
            _check(lib, getattr(lib, name + "_host")(self.N, self.K, self.D, self.B, _address(self.coeffs), _address(self.times),
                                                     *self._strides, *args))
            return
        tensor = self._kind
        args = [a.data_ptr() if isinstance(a, tensor) else a for a in tail]
        cur = ctx._enter()
        try:
            rc = getattr(ctx.lib, name)(ctx.handle, self.N, self.K, self.D, self.B, self.coeffs.data_ptr(), self.times.data_ptr(),
                                        *self._strides, *args)
        finally:
            ctx._leave(cur)
        _check(ctx.lib, rc, ctx.handle)

    def result(self, arrays, make=tuple):
        """make(arrays) (a NamedTuple's _make, or a plain tuple), without the batch axis of every array that is there when the
        call was for one trajectory."""
        if self.single:
            arrays = [a if a is None else a[0] for a in arrays]
        return make(arrays)


def sample_range(ctx: "Context", coeffs, times, t_start: float, dt: float, n_samples: int, n_derivatives: int = 5,
                 times_layout: str = "aos", want_valid: bool = False, out=None, valid=None):
    """Batched Trajectory::evaluateRange / sampleTrajectoryInRange: coeffs [B][K][D][N] and times ([B][K] 'aos' or
    [K][B] 'soa') CUDA tensors -> out [B][n_samples][n_derivatives][D] (and n_valid [B] int32).
    `out` / `valid`: caller-owned result buffers (float64 / int32 CUDA tensors of exactly that many elements on the device of
    `coeffs`, contiguous, `out` 16-byte aligned) instead of fresh allocations; `valid` implies want_valid.  The results are
    views of them in the shapes above."""
    import torch
    b = _SegmentBatch.device(ctx, coeffs, times, times_layout)
    bsz = b.B
    shape = (bsz, n_samples, n_derivatives, b.D)
    if out is None:
        out = b.empty(shape, b.f64)
    else:
        if not (out.is_cuda and out.device == coeffs.device and out.dtype == torch.float64):
            raise ValueError("sample_range: `out` must be a float64 tensor on the device of `coeffs`")
        if out.numel() != bsz * n_samples * n_derivatives * b.D or not out.is_contiguous():
            raise ValueError("sample_range: `out` must be contiguous with %d x %d x %d x %d elements" % shape)
        if out.data_ptr() % 16:
            raise ValueError("sample_range: `out` must be 16-byte aligned")
        out = out.view(shape)
    if valid is None:
        valid = b.empty((bsz,), b.i32, want_valid)
    else:
        if not (valid.is_cuda and valid.device == coeffs.device and valid.dtype == torch.int32):
            raise ValueError("sample_range: `valid` must be an int32 tensor on the device of `coeffs`")
        if valid.numel() != bsz or not valid.is_contiguous():
            raise ValueError("sample_range: `valid` must be contiguous with %d elements" % bsz)
        valid = valid.view((bsz,))
        want_valid = True
    b.call("mtg_sample_range", float(t_start), float(dt), n_samples, n_derivatives, out, valid)
    return (out, valid) if want_valid else out


def minmax_magnitude(ctx: "Context", coeffs, times, derivative: int, dimensions: Optional[Sequence[int]] = None,
                     times_layout: str = "aos"):
    """Batched Trajectory::computeMinMaxMagnitude: coeffs [B][K][D][N], times ([B][K] 'aos' / [K][B] 'soa') CUDA
    tensors -> (segment_minmax [B][K][4], trajectory_minmax [B][4], trajectory_segment_idx [B][2] int32); the four
    columns are (t_min, v_min, t_max, v_max) with segment-local times."""
    b = _SegmentBatch.device(ctx, coeffs, times, times_layout)
    mask = 0
    for d in (dimensions if dimensions is not None else range(b.D)):
        if d < 0 or d >= b.D:
            raise MtgError(-1, "dimension %d out of bounds [0..%d]" % (d, b.D - 1))
        mask |= 1 << d
    seg = b.empty((b.B, b.K, 4), b.f64)
    traj = b.empty((b.B, 4), b.f64)
    idx = b.empty((b.B, 2), b.i32)
    b.call("mtg_minmax_magnitude", int(derivative), mask, seg, traj, idx)
    return seg, traj, idx


class AxisMinMax(NamedTuple):
    """segment [B][K][D][n][4], trajectory [B][D][n][4] or None, trajectory_segment_idx [B][D][n][2] int32 or None; the four
    columns are (t_min, v_min, t_max, v_max) with segment-local times, n the orders asked for."""
    segment: object
    trajectory: object
    trajectory_segment_idx: object


def _minmax_axes(b: _SegmentBatch, derivative_first, n_derivatives, want_trajectory) -> AxisMinMax:
    nd = int(n_derivatives)
    if nd < 1 or nd > 5:
        raise MtgError(-1, "n_derivatives must be in [1, 5]")
    seg = b.empty((b.B, b.K, b.D, nd, 4), b.f64)
    traj = b.empty((b.B, b.D, nd, 4), b.f64, want_trajectory)
    idx = b.empty((b.B, b.D, nd, 2), b.i32, want_trajectory)
    b.call("mtg_minmax_axes", int(derivative_first), nd, seg, traj, idx)
    return b.result((seg, traj, idx), AxisMinMax._make)


def minmax_axes(ctx: "Context", coeffs, times, derivative_first: int = 0, n_derivatives: int = 1, times_layout: str = "aos",
                want_trajectory: bool = True) -> AxisMinMax:
    """Batched Polynomial::computeMinMax: the signed minimum and maximum of every axis over every segment, for the orders
    derivative_first .. derivative_first + n_derivatives - 1 (0 = position .. 4 = snap) from one root search per axis.  coeffs
    [B][K][D][N], times ([B][K] 'aos' / [K][B] 'soa') CUDA float64 tensors.  A row with a NaN candidate is (0, NaN, 0, NaN)."""
    return _minmax_axes(_SegmentBatch.device(ctx, coeffs, times, times_layout), derivative_first, n_derivatives, want_trajectory)


def minmax_axes_host(coeffs, times, derivative_first: int = 0, n_derivatives: int = 1, times_layout: str = "aos",
                     want_trajectory: bool = True) -> AxisMinMax:
    """The same on numpy arrays through the library's host build of the same code (no context, no device): coeffs
    [B][K][D][N] or one trajectory [K][D][N] (then the results come without the batch axis)."""
    return _minmax_axes(_SegmentBatch.host(coeffs, times, times_layout), derivative_first, n_derivatives, want_trajectory)


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
    b = _SegmentBatch.device(ctx, coeffs, times, times_layout)
    need = 8 * b.B * (b.K + 1)
    if workspace is None:
        workspace = b.empty((need,), b.f64)
    elif b.extra(workspace, "workspace").numel() < need:
        raise MtgError(-1, "workspace must hold 8 B (K + 1) = %d values" % need)
    scaling = b.empty((b.B,), b.f64)
    within = b.empty((b.B,), b.i32)
    b.call("mtg_scale_segment_times_to_meet_constraints", float(v_max), float(a_max), int(max_iterations), workspace, scaling, within)
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


def _input_feasibility(b: _SegmentBatch, name: str, constraints, want_segments, want_bounds, want_sections=None):
    """Both input-feasibility checkers: the recursive one (want_sections not None) has one more output."""
    traj = b.empty((b.B,), b.i32)
    first = b.empty((b.B,), b.i32)
    seg = b.empty((b.B, b.K), b.i32, want_segments)
    bounds = b.empty((b.B, b.K, 6), b.f64, want_bounds)
    out = [traj, first, seg, bounds]
    if want_sections is not None:
        out.append(b.empty((b.B, b.K), b.i32, want_sections))
    c = constraints.to_c()
    b.call(name, ctypes.byref(c), *out)
    return b.result(out)


def check_input_feasibility(ctx: "Context", coeffs, times, constraints: InputConstraints, times_layout: str = "aos",
                            want_segments: bool = True, want_bounds: bool = True):
    """Batched FeasibilityAnalytic::checkInputFeasibilityTrajectory: coeffs [B][K][D][N], times ([B][K] 'aos' / [K][B] 'soa')
    CUDA tensors -> (trajectory_result [B] int32, first_failing_segment [B] int32 (-1: none), segment_result [B][K] int32 or
    None, segment_bounds [B][K][6] or None: thrust min, thrust max, velocity max, whole-segment roll/pitch bound, |yaw rate|
    max, |yaw acceleration| max; NaN where not computed).  Result codes: InputFeasibilityResult."""
    return _input_feasibility(_SegmentBatch.device(ctx, coeffs, times, times_layout), "mtg_check_input_feasibility", constraints,
                              want_segments, want_bounds)


def check_input_feasibility_host(coeffs, times, constraints: InputConstraints, times_layout: str = "aos"):
    """The same check on numpy arrays through the library's host build of the same code (no context, no device): coeffs
    [B][K][D][N] or one trajectory [K][D][N]; returns numpy (trajectory_result, first_failing_segment, segment_result,
    segment_bounds), shaped as the device form's (without the batch axis for one trajectory)."""
    return _input_feasibility(_SegmentBatch.host(coeffs, times, times_layout), "mtg_check_input_feasibility", constraints, True, True)


def check_input_feasibility_recursive(ctx: "Context", coeffs, times, constraints: InputConstraints, times_layout: str = "aos",
                                      want_segments: bool = True, want_bounds: bool = True, want_sections: bool = False):
    """Batched FeasibilityRecursive::checkInputFeasibilityTrajectory (Mueller's recursive test on single-axis extrema, the cheap
    and conservative checker): the arguments of check_input_feasibility -> (trajectory_result [B] int32, first_failing_segment
    [B] int32 (-1: none), segment_result [B][K] int32 or None, segment_bounds [B][K][6] or None: f_lower_bound, f_upper_bound,
    v_upper_bound and roll/pitch bound of the whole-segment section [0, T], |yaw rate| max, |yaw acceleration| max; NaN where
    not computed, segment_sections [B][K] int32 or None: the sections the walk examined).  constraints.min_section_time_s is
    FeasibilityRecursive::Settings' value.  Result codes: InputFeasibilityResult."""
    return _input_feasibility(_SegmentBatch.device(ctx, coeffs, times, times_layout), "mtg_check_input_feasibility_recursive",
                              constraints, want_segments, want_bounds, bool(want_sections))


def check_input_feasibility_recursive_host(coeffs, times, constraints: InputConstraints, times_layout: str = "aos"):
    """The same check on numpy arrays through the library's host build of the same code (no context, no device): coeffs
    [B][K][D][N] or one trajectory [K][D][N]; returns numpy (trajectory_result, first_failing_segment, segment_result,
    segment_bounds, segment_sections), shaped as the device form's (without the batch axis for one trajectory)."""
    return _input_feasibility(_SegmentBatch.host(coeffs, times, times_layout), "mtg_check_input_feasibility_recursive", constraints,
                              True, True, True)


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


def _half_plane_feasibility(b: _SegmentBatch, planes, want_clearance) -> HalfPlaneFeasibilityResult:
    planes = b.extra(planes, "planes")
    p, psb, psk = _plane_strides(tuple(planes.shape), b.B, b.K)
    feas = b.empty((b.B,), b.i32)
    fseg = b.empty((b.B,), b.i32)
    fplane = b.empty((b.B,), b.i32)
    seg_c = b.empty((b.B, b.K), b.f64, want_clearance)
    traj_c = b.empty((b.B,), b.f64, want_clearance)
    b.call("mtg_check_half_plane_feasibility", planes, p, psb, psk, feas, fseg, fplane, seg_c, traj_c)
    return b.result((feas, fseg, fplane, seg_c, traj_c), HalfPlaneFeasibilityResult._make)


def check_half_plane_feasibility(ctx: "Context", coeffs, times, planes, times_layout: str = "aos",
                                 want_clearance: bool = True) -> HalfPlaneFeasibilityResult:
    """Batched FeasibilityBase::checkHalfPlaneFeasibility(Trajectory): coeffs [B][K][D][N], times ([B][K] 'aos' / [K][B] 'soa')
    and planes ([P][4], [K][P][4] or [B][K][P][4] rows of (unit normal, offset), see half_planes) as CUDA float64 tensors.
    A plane fails a segment iff n . p(t) - offset <= 0 at t = 0, T or a critical point of the projection."""
    return _half_plane_feasibility(_SegmentBatch.device(ctx, coeffs, times, times_layout), planes, want_clearance)


def check_half_plane_feasibility_host(coeffs, times, planes, times_layout: str = "aos") -> HalfPlaneFeasibilityResult:
    """The same check on numpy arrays through the library's host build of the same code (no context, no device): coeffs
    [B][K][D][N] or one trajectory [K][D][N] (then planes [P][4] or [K][P][4], results without the batch axis).  Normals
    that are not of unit length raise."""
    return _half_plane_feasibility(_SegmentBatch.host(coeffs, times, times_layout), planes, True)


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


def _obstacle_clearance(b: _SegmentBatch, obstacles, inflation, want_clearance) -> ObstacleClearanceResult:
    obstacles = b.extra(obstacles, "obstacles")
    m, osb = _obstacle_stride(tuple(obstacles.shape), b.B)
    feas = b.empty((b.B,), b.i32)
    fseg = b.empty((b.B,), b.i32)
    fobs = b.empty((b.B,), b.i32)
    seg_c = b.empty((b.B, b.K), b.f64, want_clearance)
    seg_o = b.empty((b.B, b.K), b.i32, want_clearance)
    seg_t = b.empty((b.B, b.K), b.f64, want_clearance)
    traj_c = b.empty((b.B,), b.f64, want_clearance)
    b.call("mtg_check_obstacle_clearance", obstacles, m, osb, float(inflation), feas, fseg, fobs, seg_c, seg_o, seg_t, traj_c)
    return b.result((feas, fseg, fobs, seg_c, seg_o, seg_t, traj_c), ObstacleClearanceResult._make)


def check_obstacle_clearance(ctx: "Context", coeffs, times, obstacles, inflation: float = 0.0, times_layout: str = "aos",
                             want_clearance: bool = True) -> ObstacleClearanceResult:
    """Batched clearance of solved trajectories from a set of spheres: coeffs [B][K][D][N] (D = 3 or 4), times ([B][K] 'aos' /
    [K][B] 'soa') and obstacles ([M][4] or [B][M][4] rows of (cx, cy, cz, r), see sphere_obstacles) as CUDA float64 tensors.
    An obstacle fails a segment iff not ||p(t) - c|| - r - inflation > 0 at t = 0, T or a critical point of the distance."""
    return _obstacle_clearance(_SegmentBatch.device(ctx, coeffs, times, times_layout), obstacles, inflation, want_clearance)


def check_obstacle_clearance_host(coeffs, times, obstacles, inflation: float = 0.0,
                                  times_layout: str = "aos") -> ObstacleClearanceResult:
    """The same check on numpy arrays through the library's host build of the same code (no context, no device): coeffs
    [B][K][D][N] or one trajectory [K][D][N] (then obstacles [M][4], results without the batch axis).  A radius that is
    negative or not finite raises."""
    return _obstacle_clearance(_SegmentBatch.host(coeffs, times, times_layout), obstacles, inflation, True)


class TrajectorySeparationResult(NamedTuple):
    """pair_feasible [P] int32 (1 / 0), first_failing_segment_a / _b [P] int32 (the earliest failing piece, -1: none),
    pair_separation [P] (minimum over the common flight time of ||pA(t) - pB(t)|| - min_separation; +inf if the two never fly at the
    same time, a NaN wins), pair_closest_time [P] (GLOBAL time of that minimum, NaN: none), pair_closest_segment_a / _b [P] int32,
    and per segment of A: segment_separation [P][Ka], segment_closest_time [P][Ka], segment_closest_segment_b [P][Ka] int32,
    segment_pieces [P][Ka] int32 (the pieces between merged breakpoints the segment was cut into).  The last seven are None if
    the closest approach was not asked for."""
    pair_feasible: object
    first_failing_segment_a: object
    first_failing_segment_b: object
    pair_separation: object
    pair_closest_time: object
    pair_closest_segment_a: object
    pair_closest_segment_b: object
    segment_separation: object
    segment_closest_time: object
    segment_closest_segment_b: object
    segment_pieces: object


def all_pairs(n: int) -> np.ndarray:
    """Every unordered pair of n trajectories: [n (n - 1) / 2][2] int32 rows (i, j) with i < j, in lexicographic order -- the pair
    list of a swarm checked against itself."""
    i, j = np.triu_indices(int(n), 1)
    return np.ascontiguousarray(np.stack([i, j], axis=1).astype(np.int32))


def _trajectory_separation(a: _SegmentBatch, b: _SegmentBatch, pairs, min_separation, start_a, start_b,
                           want_closest) -> TrajectorySeparationResult:
    if a.single or b.single:
        _bad("coeffs must be [B][K][D][N] on both sides")
    if (a.N, a.D) != (b.N, b.D):
        _bad("both sides must have the same dimension and number of coefficients")
    if a.ctx is not None and b.coeffs.device != a.coeffs.device:
        _bad("both sides must be on the same device")
    starts = []
    for side, start, what in ((a, start_a, "start_a"), (b, start_b, "start_b")):
        if start is not None:
            start = a.extra(start, what)
            if tuple(start.shape) != (side.B,):
                _bad("%s must hold one start time per trajectory (%d)" % (what, side.B))
        starts.append(start)
    pairs = a.extra(pairs, "pairs", "int32")
    if len(pairs.shape) != 2 or pairs.shape[1] != 2:
        _bad("pairs must be [P][2]")
    n = int(pairs.shape[0])
    out = [a.empty((n,), a.i32), a.empty((n,), a.i32), a.empty((n,), a.i32), a.empty((n,), a.f64), a.empty((n,), a.f64, want_closest),
           a.empty((n,), a.i32, want_closest), a.empty((n,), a.i32, want_closest), a.empty((n, a.K), a.f64, want_closest),
           a.empty((n, a.K), a.f64, want_closest), a.empty((n, a.K), a.i32, want_closest), a.empty((n, a.K), a.i32, want_closest)]
    ctx = a.ctx
    if ctx is None:
        addr = lambda x: None if x is None else _address(x)
    else:
        addr = lambda x: None if x is None else x.data_ptr()
    args = [a.N, a.D]
    for side, start in zip((a, b), starts):
        args += [side.K, side.B, addr(side.coeffs), addr(side.times), *side._strides, addr(start)]
    args += [n, addr(pairs), float(min_separation)] + [addr(x) for x in out]
    if ctx is None:
        lib = L.load()
        _check(lib, lib.mtg_check_trajectory_separation_host(*args))
    else:
        cur = ctx._enter()
        try:
            rc = ctx.lib.mtg_check_trajectory_separation(ctx.handle, *args)
        finally:
            ctx._leave(cur)
        _check(ctx.lib, rc, ctx.handle)
    return TrajectorySeparationResult._make(out)


def check_trajectory_separation(ctx: "Context", coeffs_a, times_a, coeffs_b, times_b, pairs, min_separation: float, start_a=None,
                                start_b=None, times_layout: str = "aos", want_closest: bool = True) -> TrajectorySeparationResult:
    """Batched separation of solved trajectories from EACH OTHER: side A coeffs_a [Ba][Ka][D][N] with times_a, side B coeffs_b
    [Bb][Kb][D][N] with times_b (D = 3 or 4; both 'aos' [B][K] or both 'soa' [K][B]; the two sides may be the same tensors),
    start_a [Ba] / start_b [Bb] the global time at which each trajectory starts (None: 0), pairs [P][2] int32 rows of (index into
    A, index into B), see all_pairs -- CUDA tensors.  A pair fails iff not ||pA(t) - pB(t)|| - min_separation > 0 at a breakpoint of
    either side or a critical point of the distance within the time both fly; a pair that never flies at the same time is feasible
    with separation +inf.  A pair with an index out of range, a negative or non-finite segment time or a non-finite start is
    infeasible with NaN separation.  include/mtg_hip.h has every rule."""
    return _trajectory_separation(_SegmentBatch.device(ctx, coeffs_a, times_a, times_layout),
                                  _SegmentBatch.device(ctx, coeffs_b, times_b, times_layout), pairs, min_separation, start_a, start_b,
                                  want_closest)


def check_trajectory_separation_host(coeffs_a, times_a, coeffs_b, times_b, pairs, min_separation: float, start_a=None, start_b=None,
                                     times_layout: str = "aos", want_closest: bool = True) -> TrajectorySeparationResult:
    """The same check on numpy arrays through the library's host build of the same code (no context, no device).  Here a pair index
    out of range raises."""
    return _trajectory_separation(_SegmentBatch.host(coeffs_a, times_a, times_layout), _SegmentBatch.host(coeffs_b, times_b, times_layout),
                                  pairs, min_separation, start_a, start_b, want_closest)


def keep_out_boxes(centers, sizes) -> np.ndarray:
    """n boxes as keep-out zones: centers [n][3] and sizes [n][3] (or one [3] for all) -> [n][6][4], bounding_box_half_planes per
    box in its own plane order and signs.  A size that is not positive or not finite raises."""
    lib = L.load()
    centers = np.ascontiguousarray(centers, dtype=np.float64)
    if centers.ndim != 2 or centers.shape[1] != 3:
        raise MtgError(-1, "centers must be [n][3]")
    try:
        sizes = np.ascontiguousarray(np.broadcast_to(np.asarray(sizes, dtype=np.float64), centers.shape))
    except ValueError:
        raise MtgError(-1, "sizes must be [n][3] or [3]") from None
    out = np.empty((centers.shape[0], 6, 4), dtype=np.float64)
    _check(lib, lib.mtg_keep_out_boxes(centers.shape[0], centers.ctypes.data, sizes.ctypes.data, out.ctypes.data))
    return out


class KeepOutResult(NamedTuple):
    """trajectory_feasible [B] int32 (1 / 0), first_failing_segment [B] int32 (-1: none), first_failing_zone [B] int32 (-1: none),
    segment_clearance [B][K], segment_nearest_zone [B][K] int32, segment_closest_time [B][K], trajectory_clearance [B] (minimum
    over t of max_j (offset_j - n_j . p(t)) - inflation; a NaN wins); the last four None if not asked for."""
    trajectory_feasible: object
    first_failing_segment: object
    first_failing_zone: object
    segment_clearance: object
    segment_nearest_zone: object
    segment_closest_time: object
    trajectory_clearance: object


def _zone_shape(shape, bsz: int):
    """[P][4]: one zone; [M][P][4]: one set for every trajectory; [B][M][P][4]: a set per trajectory."""
    if len(shape) not in (2, 3, 4) or shape[-1] != 4:
        raise MtgError(-1, "zones must be [P][4], [M][P][4] or [B][M][P][4]")
    p = int(shape[-2])
    m = int(shape[-3]) if len(shape) >= 3 else 1
    if len(shape) == 4 and shape[0] != bsz:
        raise MtgError(-1, "zones: the batch axis must match coeffs")
    return m, p, (4 * p * m if len(shape) == 4 else 0)


def _keep_out_zones(b: _SegmentBatch, zones, inflation, want_clearance) -> KeepOutResult:
    zones = b.extra(zones, "zones")
    m, p, zsb = _zone_shape(tuple(zones.shape), b.B)
    feas = b.empty((b.B,), b.i32)
    fseg = b.empty((b.B,), b.i32)
    fzone = b.empty((b.B,), b.i32)
    seg_c = b.empty((b.B, b.K), b.f64, want_clearance)
    seg_z = b.empty((b.B, b.K), b.i32, want_clearance)
    seg_t = b.empty((b.B, b.K), b.f64, want_clearance)
    traj_c = b.empty((b.B,), b.f64, want_clearance)
    b.call("mtg_check_keep_out_zones", zones, m, p, zsb, float(inflation), feas, fseg, fzone, seg_c, seg_z, seg_t, traj_c)
    return b.result((feas, fseg, fzone, seg_c, seg_z, seg_t, traj_c), KeepOutResult._make)


def check_keep_out_zones(ctx: "Context", coeffs, times, zones, inflation: float = 0.0, times_layout: str = "aos",
                         want_clearance: bool = True) -> KeepOutResult:
    """Batched check that solved trajectories stay OUTSIDE a set of convex zones (boxes, prisms): coeffs [B][K][D][N] (D = 3 or
    4), times ([B][K] 'aos' / [K][B] 'soa') and zones ([M][P][4] or [B][M][P][4] rows of (unit normal pointing into the zone,
    offset), see keep_out_boxes; one [P][4] array, as bounding_box_half_planes returns it, is one zone) as CUDA float64 tensors.
    A zone fails a segment iff not min_t max_j (offset_j - n_j . p(t)) - inflation > 0."""
    return _keep_out_zones(_SegmentBatch.device(ctx, coeffs, times, times_layout), zones, inflation, want_clearance)


def check_keep_out_zones_host(coeffs, times, zones, inflation: float = 0.0, times_layout: str = "aos") -> KeepOutResult:
    """The same check on numpy arrays through the library's host build of the same code (no context, no device): coeffs
    [B][K][D][N] or one trajectory [K][D][N] (then zones [P][4] or [M][P][4], results without the batch axis).  A normal that
    is not of unit length or an offset that is not finite raises."""
    return _keep_out_zones(_SegmentBatch.host(coeffs, times, times_layout), zones, inflation, True)


_INTERPOLATION = {"nearest": 0, "trilinear": 1}


class DistanceField:
    """A voxel grid of distances (an ESDF, an inflated occupancy map): distances float32 [nz][ny][nx], x fastest (a CUDA tensor
    for check_distance_field, a numpy array for check_distance_field_host), origin = position of the CENTRE of voxel (0, 0, 0),
    voxel_size h > 0, outside_distance = the value of a sample outside the grid (0: unknown space is an obstacle, inf: free;
    not NaN), interpolation 'trilinear' or 'nearest'."""
    __slots__ = ("distances", "origin", "voxel_size", "outside_distance", "interpolation")

    def __init__(self, distances, origin, voxel_size: float, outside_distance: float = 0.0, interpolation: str = "trilinear"):
        try:
            origin = tuple(float(x) for x in origin)
        except TypeError:
            origin = ()
        if len(origin) != 3:
            _bad("origin must hold 3 numbers")
        if interpolation not in _INTERPOLATION:
            _bad("interpolation must be 'trilinear' or 'nearest'")
        self.distances, self.origin, self.voxel_size = distances, origin, float(voxel_size)
        self.outside_distance, self.interpolation = float(outside_distance), interpolation

    @classmethod
    def from_corner(cls, distances, min_corner, voxel_size: float, outside_distance: float = 0.0, interpolation: str = "trilinear"):
        """For maps whose origin is the lower CORNER of voxel (0, 0, 0): its centre is the corner plus h / 2 on every axis."""
        try:
            origin = [float(x) + 0.5 * float(voxel_size) for x in min_corner]
        except TypeError:
            origin = ()
        return cls(distances, origin, voxel_size, outside_distance, interpolation)

    def lipschitz_bound(self) -> float:
        """A rigorous Lipschitz constant of the trilinear interpolant, the `lipschitz` of certify_distance_field: per cell the
        largest absolute difference over its four x-, y- and z-edges (gx, gy, gz), then the maximum over the cells of
        sqrt(gx^2 + gy^2 + gz^2) / h, rounded up.  A numpy grid goes through the library's host function; a CUDA tensor through
        the same formula as torch operations in float64, times 1 + 2^-40.  Non-finite if a voxel is."""
        grid = self.distances
        if len(grid.shape) != 3 or min(int(n) for n in grid.shape) < 2:
            _bad("distances must be [nz][ny][nx] with every axis >= 2")
        if isinstance(grid, np.ndarray):
            if grid.dtype != np.float32 or not grid.flags.c_contiguous:
                _bad("distances must be a contiguous float32 array")
            lib = L.load()
            nz, ny, nx = (int(n) for n in grid.shape)
            c = L.DistanceFieldC(grid.ctypes.data, nx, ny, nz, (ctypes.c_double * 3)(*self.origin), self.voxel_size,
                                 self.outside_distance, _INTERPOLATION[self.interpolation])
            out = ctypes.c_double()
            _check(lib, lib.mtg_distance_field_lipschitz_host(ctypes.byref(c), ctypes.byref(out)))
            return out.value
        import torch
        if not (self.voxel_size > 0.0):
            _bad("voxel_size must be > 0")
        g = grid.to(torch.float64)
        dx, dy, dz = (g[:, :, 1:] - g[:, :, :-1]).abs(), (g[:, 1:, :] - g[:, :-1, :]).abs(), (g[1:, :, :] - g[:-1, :, :]).abs()
        # the four parallel edges of a cell: the maximum over the two neighbours along each of the other two axes
        gx = torch.maximum(torch.maximum(dx[:-1, :-1], dx[:-1, 1:]), torch.maximum(dx[1:, :-1], dx[1:, 1:]))
        gy = torch.maximum(torch.maximum(dy[:-1, :, :-1], dy[:-1, :, 1:]), torch.maximum(dy[1:, :, :-1], dy[1:, :, 1:]))
        gz = torch.maximum(torch.maximum(dz[:, :-1, :-1], dz[:, :-1, 1:]), torch.maximum(dz[:, 1:, :-1], dz[:, 1:, 1:]))
        worst = torch.sqrt(gx * gx + gy * gy + gz * gz).amax()       # (torch.maximum and amax propagate a NaN)
        return float(worst) / self.voxel_size * (1.0 + 2.0 ** -40)


class DistanceFieldResult(NamedTuple):
    """trajectory_feasible [B] int32 (1 / 0), first_failing_segment [B] int32 (-1: none), segment_clearance [B][K],
    segment_closest_sample [B][K] int32, segment_first_failing_sample [B][K] int32 (-1: none), segment_samples [B][K] int32 (S;
    -1: more than max_samples, not sampled), trajectory_clearance [B] (minimum over the samples of distance - inflation; a NaN
    wins), and two times derived from them: segment_closest_time [B][K] (local time of the closest sample: T for sample S - 1,
    else i dt; NaN if not sampled) and first_failing_time [B] (local time of the first failing sample of the first failing
    segment; NaN for a feasible trajectory or a segment that was not sampled).  Everything per segment, and the two times, are
    None if the segments were not asked for."""
    trajectory_feasible: object
    first_failing_segment: object
    segment_clearance: object
    segment_closest_sample: object
    segment_first_failing_sample: object
    segment_samples: object
    trajectory_clearance: object
    segment_closest_time: object
    first_failing_time: object


def _sample_times(b: _SegmentBatch, index, samples, times, dt):
    """where(i == S - 1, T, i dt), NaN where i < 0, as operations on whole arrays of either form."""
    if b.ctx is None:
        return np.where(index < 0, np.nan, np.where(index == samples - 1, times, index * dt))
    import torch
    t = torch.where(index == samples - 1, times, index.to(times.dtype) * dt)
    return torch.where(index < 0, torch.full_like(t, float("nan")), t)


def _field_struct(b: _SegmentBatch, field):
    """(grid, the mtg_distance_field of a DistanceField) for either form; grid keeps the voxels alive during the call."""
    if not isinstance(field, DistanceField):
        _bad("field must be a DistanceField")
    grid = field.distances
    if b.ctx is None and not isinstance(grid, np.ndarray):
        _bad("distances must be a numpy array")
    if b.ctx is not None and not isinstance(grid, b._kind):
        _bad("distances must be a tensor")
    if b.ctx is None and (grid.dtype != np.float32 or not grid.flags.c_contiguous):
        _bad("distances must be a contiguous float32 array")
    if len(grid.shape) != 3:
        _bad("distances must be [nz][ny][nx]")
    grid = b.extra(grid, "distances", "float32")
    nz, ny, nx = (int(n) for n in grid.shape)
    if nx * ny * nz == 0 or nx * ny * nz > 2**31 - 1:
        _bad("distances must hold 1 .. 2^31 - 1 voxels")
    return grid, L.DistanceFieldC(grid.ctypes.data if b.ctx is None else grid.data_ptr(), nx, ny, nz, (ctypes.c_double * 3)(*field.origin),
                                  field.voxel_size, field.outside_distance, _INTERPOLATION[field.interpolation])


def _distance_field(b: _SegmentBatch, field, dt, inflation, max_samples, want_segments) -> DistanceFieldResult:
    grid, c = _field_struct(b, field)
    feas = b.empty((b.B,), b.i32)
    fseg = b.empty((b.B,), b.i32)
    seg_c = b.empty((b.B, b.K), b.f64, want_segments)
    seg_i = b.empty((b.B, b.K), b.i32, want_segments)
    seg_f = b.empty((b.B, b.K), b.i32, want_segments)
    seg_s = b.empty((b.B, b.K), b.i32, want_segments)
    traj_c = b.empty((b.B,), b.f64)
    b.call("mtg_check_distance_field", ctypes.byref(c), float(dt), int(max_samples), float(inflation), feas, fseg, seg_c, seg_i, seg_f,
           seg_s, traj_c)
    seg_t = fail_t = None
    if want_segments:
        times = b.times.reshape(b.B, b.K) if b._strides[1] == 1 else b.times.reshape(b.K, b.B).T
        seg_t = _sample_times(b, seg_i, seg_s, times, float(dt))
        k = fseg.clip(0)[:, None]
        if b.ctx is None:
            pick = lambda a: np.take_along_axis(a, k, 1)[:, 0]
            fail_t = np.where(fseg < 0, np.nan, _sample_times(b, pick(seg_f), pick(seg_s), pick(times), float(dt)))
        else:
            import torch
            pick = lambda a: torch.gather(a, 1, k.long())[:, 0]
            fail_t = _sample_times(b, pick(seg_f), pick(seg_s), pick(times), float(dt))
            fail_t = torch.where(fseg < 0, torch.full_like(fail_t, float("nan")), fail_t)
    return b.result((feas, fseg, seg_c, seg_i, seg_f, seg_s, traj_c, seg_t, fail_t), DistanceFieldResult._make)


def check_distance_field(ctx: "Context", coeffs, times, field: DistanceField, dt: float, inflation: float = 0.0, max_samples: int = 4096,
                         times_layout: str = "aos", want_segments: bool = True) -> DistanceFieldResult:
    """Batched SAMPLED collision check of solved trajectories against a voxel grid of distances: coeffs [B][K][D][N] (D = 3 or 4),
    times ([B][K] 'aos' / [K][B] 'soa') as CUDA float64 tensors, field a DistanceField whose distances are a float32 CUDA tensor.
    Every segment is sampled at local times 0, i dt < T and T; a sample fails iff not distance(p(t)) - inflation > 0.  A segment
    with more than max_samples samples is not sampled and fails.  Between samples nothing is certified: choose dt against the
    vehicle's speed and the map's resolution.  include/mtg_hip.h has every rule."""
    return _distance_field(_SegmentBatch.device(ctx, coeffs, times, times_layout), field, dt, inflation, max_samples, want_segments)


def check_distance_field_host(coeffs, times, field: DistanceField, dt: float, inflation: float = 0.0, max_samples: int = 4096,
                              times_layout: str = "aos") -> DistanceFieldResult:
    """The same check on numpy arrays through the library's host build of the same code (no context, no device): coeffs
    [B][K][D][N] or one trajectory [K][D][N] (results then without the batch axis); field.distances a float32 numpy array."""
    return _distance_field(_SegmentBatch.host(coeffs, times, times_layout), field, dt, inflation, max_samples, True)


class CertifiedFieldResult(NamedTuple):
    """trajectory_result [B] int32 (0 COLLIDES, 1 FREE, 2 UNDECIDED_DEPTH, 3 UNDECIDED_BUDGET: the code of the first segment that is
    not FREE), first_failing_segment [B] int32 (-1: none), segment_result [B][K] int32, segment_lower_bound [B][K] (guaranteed
    lower bound of min_t distance - inflation), segment_sampled_clearance [B][K] (its upper bound: the lowest sample),
    segment_closest_time [B][K] (local time of that sample), segment_first_failing_time [B][K] (NaN: none), segment_nodes [B][K]
    int32, segment_depth [B][K] int32, trajectory_lower_bound [B], trajectory_sampled_clearance [B], lipschitz (the constant the
    call used).  Everything per segment is None if the segments were not asked for."""
    trajectory_result: object
    first_failing_segment: object
    segment_result: object
    segment_lower_bound: object
    segment_sampled_clearance: object
    segment_closest_time: object
    segment_first_failing_time: object
    segment_nodes: object
    segment_depth: object
    trajectory_lower_bound: object
    trajectory_sampled_clearance: object
    lipschitz: object


def _certify_distance_field(b: _SegmentBatch, field, lipschitz, inflation, min_depth, max_depth, max_frontier,
                            want_segments) -> CertifiedFieldResult:
    grid, c = _field_struct(b, field)
    if lipschitz is None:
        lipschitz = field.lipschitz_bound()
    res = b.empty((b.B,), b.i32)
    fseg = b.empty((b.B,), b.i32)
    seg_r = b.empty((b.B, b.K), b.i32, want_segments)
    seg_l = b.empty((b.B, b.K), b.f64, want_segments)
    seg_c = b.empty((b.B, b.K), b.f64, want_segments)
    seg_t = b.empty((b.B, b.K), b.f64, want_segments)
    seg_f = b.empty((b.B, b.K), b.f64, want_segments)
    seg_n = b.empty((b.B, b.K), b.i32, want_segments)
    seg_d = b.empty((b.B, b.K), b.i32, want_segments)
    traj_l = b.empty((b.B,), b.f64)
    traj_c = b.empty((b.B,), b.f64)
    b.call("mtg_certify_distance_field", ctypes.byref(c), float(lipschitz), int(min_depth), int(max_depth), int(max_frontier),
           float(inflation), res, fseg, seg_r, seg_l, seg_c, seg_t, seg_f, seg_n, seg_d, traj_l, traj_c)
    r = b.result((res, fseg, seg_r, seg_l, seg_c, seg_t, seg_f, seg_n, seg_d, traj_l, traj_c))
    return CertifiedFieldResult(*r, float(lipschitz))


def certify_distance_field(ctx: "Context", coeffs, times, field: DistanceField, lipschitz: Optional[float] = None, inflation: float = 0.0,
                           min_depth: int = 4, max_depth: int = 16, max_frontier: int = 1024, times_layout: str = "aos",
                           want_segments: bool = True) -> CertifiedFieldResult:
    """Batched CERTIFIED collision check of solved trajectories against a trilinear voxel grid of distances: coeffs [B][K][D][N]
    (D = 3 or 4), times ([B][K] 'aos' / [K][B] 'soa') as CUDA float64 tensors, field a DistanceField whose distances are a float32
    CUDA tensor.  Every segment is covered by an adaptive bisection of its time interval; a node is a sample at its midpoint plus
    the bound distance - inflation - lipschitz * reach over the whole node.  A verdict holds for every instant: FREE is proven,
    COLLIDES has a definite failing sample, the two UNDECIDED codes name the limit that stopped the search.  lipschitz=None
    computes field.lipschitz_bound().  include/mtg_hip.h has every rule."""
    return _certify_distance_field(_SegmentBatch.device(ctx, coeffs, times, times_layout), field, lipschitz, inflation, min_depth,
                                   max_depth, max_frontier, want_segments)


def certify_distance_field_host(coeffs, times, field: DistanceField, lipschitz: Optional[float] = None, inflation: float = 0.0,
                                min_depth: int = 4, max_depth: int = 16, max_frontier: int = 1024,
                                times_layout: str = "aos") -> CertifiedFieldResult:
    """The same check on numpy arrays through the library's host build of the same code (no context, no device): coeffs
    [B][K][D][N] or one trajectory [K][D][N] (results then without the batch axis); field.distances a float32 numpy array."""
    return _certify_distance_field(_SegmentBatch.host(coeffs, times, times_layout), field, lipschitz, inflation, min_depth, max_depth,
                                   max_frontier, True)


class CollisionCostResult(NamedTuple):
    """trajectory_cost [B] (sum of segment_cost in segment order), segment_cost [B][K] (sum over the samples of w c(d - inflation) s;
    NaN: not sampled), coeff_gradient [B][K][D][N] (the exact derivative of segment_cost with respect to coeffs, the yaw rows 0) or
    None, segment_samples [B][K] int32 (S; -1: more than max_samples, not sampled)."""
    trajectory_cost: object
    segment_cost: object
    coeff_gradient: object
    segment_samples: object


def _collision_cost(b: _SegmentBatch, field, dt, inflation, epsilon, speed_epsilon, max_samples, want_gradient) -> CollisionCostResult:
    grid, c = _field_struct(b, field)
    traj = b.empty((b.B,), b.f64)
    seg = b.empty((b.B, b.K), b.f64)
    grad = b.empty((b.B, b.K, b.D, b.N), b.f64, want_gradient)
    seg_s = b.empty((b.B, b.K), b.i32)
    b.call("mtg_collision_cost", ctypes.byref(c), float(dt), int(max_samples), float(inflation), float(epsilon), float(speed_epsilon),
           seg, traj, grad, seg_s)
    return b.result((traj, seg, grad, seg_s), CollisionCostResult._make)


def collision_cost(ctx: "Context", coeffs, times, field: DistanceField, dt: float, *, inflation: float = 0.0, epsilon: float,
                   speed_epsilon: float = 1e-3, max_samples: int = 4096, want_gradient: bool = True,
                   times_layout: str = "aos") -> CollisionCostResult:
    """Batched distance-field collision cost of solved trajectories and its gradient with respect to the polynomial coefficients,
    the map term of a CHOMP-style objective: coeffs [B][K][D][N] (D = 3 or 4), times ([B][K] 'aos' / [K][B] 'soa') as CUDA float64
    tensors, field a trilinear DistanceField whose distances are a float32 CUDA tensor.  Every segment is sampled at local times 0,
    i dt < T and T with trapezoid weights w; a sample adds w c(d(p) - inflation) sqrt(|v|^2 + speed_epsilon^2) with the CHOMP potential
    c (epsilon / 2 - x below 0, (x - epsilon)^2 / (2 epsilon) up to epsilon, 0 beyond).  The gradient is the exact derivative of
    that sum.  A segment with more than max_samples samples is not sampled: NaN.  include/mtg_hip.h has every rule."""
    return _collision_cost(_SegmentBatch.device(ctx, coeffs, times, times_layout), field, dt, inflation, epsilon, speed_epsilon,
                           max_samples, want_gradient)


def collision_cost_host(coeffs, times, field: DistanceField, dt: float, *, inflation: float = 0.0, epsilon: float,
                        speed_epsilon: float = 1e-3, max_samples: int = 4096, want_gradient: bool = True,
                        times_layout: str = "aos") -> CollisionCostResult:
    """The same on numpy arrays through the library's host build of the same code, with the device's order of every sum (no
    context, no device): coeffs [B][K][D][N] or one trajectory [K][D][N] (results then without the batch axis); field.distances a
    float32 numpy array."""
    return _collision_cost(_SegmentBatch.host(coeffs, times, times_layout), field, dt, inflation, epsilon, speed_epsilon, max_samples,
                           want_gradient)


def _magnitude_soft_cost(b: _SegmentBatch, params):
    nc = params.n_constraints
    cost = b.empty((b.B,), b.f64)
    maxima = b.empty((b.B, nc), b.f64)
    violations = b.empty((b.B, nc), b.f64)
    c = params.to_c()
    b.call("mtg_magnitude_soft_cost", ctypes.byref(c), cost, maxima if nc else None, violations if nc else None)
    return b.result((cost, maxima, violations))


def magnitude_soft_cost(ctx, coeffs, times, params: TimeObjectiveParams, times_layout: str = "aos"):
    """The maxima + soft-cost stage alone (the third term of getTotalCostWithSoftConstraints): coeffs [B][K][D][N], times ([B][K]
    'aos' / [K][B] 'soa') CUDA tensors -> (cost_soft [B], maxima [B][n_constraints], violations [B][n_constraints])."""
    return _magnitude_soft_cost(_SegmentBatch.device(ctx, coeffs, times, times_layout), params)


def magnitude_soft_cost_host(coeffs, times, params: TimeObjectiveParams, times_layout: str = "aos"):
    """The same on numpy arrays through the library's host build of the same lane code (no context, no device): coeffs
    [B][K][D][N] or one trajectory [K][D][N]; returns numpy (cost_soft, maxima, violations)."""
    return _magnitude_soft_cost(_SegmentBatch.host(coeffs, times, times_layout), params)
