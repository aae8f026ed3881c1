"""The nonlinear time objective with soft constraints for a batch (C ABI: mtg_time_objective, mtg_magnitude_soft_cost[_host]) and
a deliberately small pattern search over the segment times on top of it.

What the reference minimises per trajectory (PolynomialOptimizationNonLinear<N>, impl/polynomial_optimization_nonlinear_impl.h):
objectiveFunctionTime :556-615 and objectiveFunctionTimeAndConstraints :660-742 = cost_trajectory + cost_time + cost_soft.  Here
one call evaluates it for every trajectory of a batch; pattern_search_segment_times shows the entry in use -- all candidates of an
iteration in ONE call -- and is plumbing over the kernel, not a claim to be a good optimiser.
"""
from __future__ import annotations

import ctypes
import enum
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L
from .core import MtgError, Plan, _check
from .segment_checks import magnitude_soft_cost, magnitude_soft_cost_host  # noqa: F401  (the maxima + soft-cost stage alone)

MAX_MAGNITUDE_CONSTRAINTS = 4


class TimeCostKind(enum.IntEnum):
    """NonlinearOptimizationParameters::TimeAllocMethod (polynomial_optimization_nonlinear.h:88-95)."""
    kSquaredTime = 0
    kRichterTime = 1
    kMellingerOuterLoop = 2
    kSquaredTimeAndConstraints = 3
    kRichterTimeAndConstraints = 4


class TimeObjectiveParams:
    """The objective's share of NonlinearOptimizationParameters, with the reference's defaults, and the ordered list of
    maximum-magnitude constraints (addMaximumMagnitudeConstraint(derivative, value)); derivatives 1 .. N/2 - 1, values > 0."""

    def __init__(self, time_cost_kind: int = TimeCostKind.kSquaredTimeAndConstraints, time_penalty: float = 500.0,
                 use_soft_constraints: bool = True, soft_constraint_weight: float = 100.0, maximum_cost: float = 1.0e12,
                 constraints: Sequence[Tuple[int, float]] = ()):
        self.time_cost_kind = int(time_cost_kind)
        self.time_penalty = float(time_penalty)
        self.use_soft_constraints = bool(use_soft_constraints)
        self.soft_constraint_weight = float(soft_constraint_weight)
        self.maximum_cost = float(maximum_cost)
        self.constraints = []
        for derivative, value in constraints:
            self.add_maximum_magnitude_constraint(derivative, value)

    def add_maximum_magnitude_constraint(self, derivative: int, value: float):
        if len(self.constraints) >= MAX_MAGNITUDE_CONSTRAINTS:
            raise MtgError(-1, "at most %d maximum-magnitude constraints" % MAX_MAGNITUDE_CONSTRAINTS)
        if int(derivative) < 1 or not float(value) > 0.0:
            raise MtgError(-1, "a maximum-magnitude constraint needs a derivative >= 1 and a value > 0")
        self.constraints.append((int(derivative), float(value)))

    @property
    def n_constraints(self) -> int:
        return len(self.constraints)

    def to_c(self) -> L.TimeObjectiveParamsC:
        c = L.TimeObjectiveParamsC()
        c.time_cost_kind, c.use_soft_constraints = self.time_cost_kind, int(self.use_soft_constraints)
        c.time_penalty, c.soft_constraint_weight, c.maximum_cost = self.time_penalty, self.soft_constraint_weight, self.maximum_cost
        c.n_constraints = len(self.constraints)
        for q, (derivative, value) in enumerate(self.constraints):
            c.derivative[q], c.value[q] = derivative, value
        return c


class TimeObjectiveResult(NamedTuple):
    objective: object    # [B]; +inf where the solve flagged the trajectory
    components: object   # [B][3] = (cost_trajectory, cost_time, cost_soft)
    maxima: object       # [B][n_constraints]
    violations: object   # [B][n_constraints] = maximum - value
    coeffs: object       # [B][K][D][N]


def time_objective(plan: Plan, times, d_fixed, params: TimeObjectiveParams, d_free=None, layout: str = "aos", coeffs=None,
                   ordered: bool = True) -> TimeObjectiveResult:
    """objectiveFunctionTime (d_free None) / objectiveFunctionTimeAndConstraints (d_free given, in `layout`) for every trajectory:
    times / d_fixed float64 CUDA tensors in `layout` ('aos': [B][K], [B][D][n_fixed]; 'soa': [K][B], [D][n_fixed][B]).
    Asynchronous; flags of the solve surface at ctx.sync()."""
    import torch
    batch = times.shape[0] if layout == "aos" else times.shape[1]
    assert times.dtype == torch.float64 and times.is_cuda and times.is_contiguous()
    assert d_fixed.dtype == torch.float64 and d_fixed.is_cuda and d_fixed.is_contiguous()
    if d_free is not None:
        assert d_free.dtype == torch.float64 and d_free.is_cuda and d_free.is_contiguous()
    dev, nc = times.device, params.n_constraints
    if coeffs is None:
        coeffs = torch.empty((batch, plan.K, plan.D, plan.N), dtype=torch.float64, device=dev)
    objective = torch.empty((batch,), dtype=torch.float64, device=dev)
    components = torch.empty((batch, 3), dtype=torch.float64, device=dev)
    maxima = torch.empty((batch, nc), dtype=torch.float64, device=dev)
    violations = torch.empty((batch, nc), dtype=torch.float64, device=dev)
    lay = plan.layout(batch, layout)
    c = params.to_c()
    cur = plan.ctx._enter() if ordered else None
    rc = plan.lib.mtg_time_objective(plan.handle, batch, ctypes.byref(lay), plan._ptr(times), plan._ptr(d_fixed), plan._ptr(d_free),
                                     ctypes.byref(c), plan._ptr(coeffs), plan._ptr(objective), plan._ptr(components),
                                     plan._ptr(maxima) if nc else None, plan._ptr(violations) if nc else None)
    if ordered:
        plan.ctx._leave(cur)
    _check(plan.lib, rc, plan.ctx.handle)
    return TimeObjectiveResult(objective, components, maxima, violations, coeffs)


def time_cost_host(times, params: TimeObjectiveParams):
    """cost_time of the objective on the host (mtg_time_cost_host): times [B][K] or [K] numpy -> [B] or a float."""
    lib = L.load()
    times = np.ascontiguousarray(times, dtype=np.float64)
    single = times.ndim == 1
    if single:
        times = times[None]
    bsz, k = times.shape
    out = np.empty((bsz,), dtype=np.float64)
    c = params.to_c()
    _check(lib, lib.mtg_time_cost_host(ctypes.byref(c), k, bsz, times.ctypes.data, k, 1, out.ctypes.data))
    return float(out[0]) if single else out


class PatternSearchResult(NamedTuple):
    times: object       # [B][K]
    coeffs: object      # [B][K][D][N] at those times
    objective: object   # [B]
    history: object     # [n_iterations + 1][B]: objective of the current point before iteration i, last row after the last one,
                        # as the candidate launches evaluated it (the result's `objective` is a fresh evaluation of its own)


def pattern_search_segment_times(plan: Plan, times, d_fixed, params: TimeObjectiveParams, n_iterations: int = 12,
                                 step0: float = 0.1, lower_bound: float = 0.1) -> PatternSearchResult:
    """Coordinate pattern search on the segment times of every trajectory (AoS tensors: times [B][K], d_fixed [B][D][n_fixed]).
    Per iteration the 2K + 1 candidates of trajectory b are its current times, T_k (1 + s_b) for each k, and
    max(lower_bound, T_k (1 - s_b)) for each k; all (2K + 1) B objectives come from ONE time_objective call (candidate-major,
    d_fixed replicated once); the best candidate becomes the current point, and s_b is halved where candidate 0 wins.  A fixed
    number of iterations, nothing in the loop waits for the device."""
    import torch
    bsz, k = times.shape
    nc = 2 * k + 1
    cur = times.clone()
    step = torch.full((bsz,), float(step0), dtype=torch.float64, device=times.device)
    fixed_rep = d_fixed.unsqueeze(0).expand(nc, *d_fixed.shape).reshape(nc * bsz, *d_fixed.shape[1:]).contiguous()
    eye = torch.eye(k, dtype=torch.float64, device=times.device)
    coeffs = torch.empty((nc * bsz, plan.K, plan.D, plan.N), dtype=torch.float64, device=times.device)
    history = torch.full((n_iterations + 1, bsz), float("nan"), dtype=torch.float64, device=times.device)
    rows = torch.arange(bsz, device=times.device)
    for it in range(n_iterations):
        s = step.view(bsz, 1, 1)
        base = cur.unsqueeze(1)                                               # [B][1][K]
        up = torch.where(eye.bool().unsqueeze(0), base * (1.0 + s), base)     # [B][K][K]: row j scales T_j
        down = torch.where(eye.bool().unsqueeze(0), torch.clamp(base * (1.0 - s), min=lower_bound), base)
        cand = torch.cat([base, up, down], dim=1).transpose(0, 1).contiguous()   # [2K + 1][B][K], candidate-major
        res = time_objective(plan, cand.view(nc * bsz, k), fixed_rep, params, coeffs=coeffs)
        obj = res.objective.view(nc, bsz)
        if it == 0:
            history[0] = obj[0]
        moved, j = torch.min(obj[1:], dim=0)
        best = torch.where(moved < obj[0], j + 1, torch.zeros_like(j))         # (a tie with the current point stays there)
        cur = cand[best, rows]
        history[it + 1] = obj[best, rows]
        step = torch.where(best == 0, step * 0.5, step)
    final = time_objective(plan, cur, d_fixed, params)
    return PatternSearchResult(cur, final.coeffs, final.objective, history)
