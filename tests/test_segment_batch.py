"""The Python layer of the per-segment batch calls (mav_trajectory_generation_amd/segment_checks.py), without a device: the public
surface is what it was before the calls moved there (signatures and exported names as literal tables), the six host forms share
their handling of layouts, single trajectories and bad `times`, and the device form's validator rejects what it must -- driven with
CPU torch tensors and a stand-in context, since it looks at dtype, rank, element count, contiguity and layout before the device."""
import inspect
import types

import numpy as np
import pytest

import mav_trajectory_generation_amd as m
from mav_trajectory_generation_amd import segment_checks as sc
from test_gpu_segment_frame import inputs

# str(inspect.signature(f)) of every public function that moved, as it was in core.py / time_objective_search.py
SIGNATURES = {
    'sample_range': '(ctx: "\'Context\'", coeffs, times, t_start: \'float\', dt: \'float\', n_samples: \'int\', n_derivatives: \'int\' = 5, times_layout: \'str\' = \'aos\', want_valid: \'bool\' = False, out=None, valid=None)',
    'minmax_magnitude': '(ctx: "\'Context\'", coeffs, times, derivative: \'int\', dimensions: \'Optional[Sequence[int]]\' = None, times_layout: \'str\' = \'aos\')',
    'minmax_axes': '(ctx: "\'Context\'", coeffs, times, derivative_first: \'int\' = 0, n_derivatives: \'int\' = 1, times_layout: \'str\' = \'aos\', want_trajectory: \'bool\' = True) -> \'AxisMinMax\'',
    'minmax_axes_host': "(coeffs, times, derivative_first: 'int' = 0, n_derivatives: 'int' = 1, times_layout: 'str' = 'aos', want_trajectory: 'bool' = True) -> 'AxisMinMax'",
    'bounding_boxes': '(ctx: "\'Context\'", coeffs, times, times_layout: \'str\' = \'aos\', margin: \'float\' = 0.0)',
    'scale_segment_times_to_meet_constraints': '(ctx: "\'Context\'", coeffs, times, v_max: \'float\', a_max: \'float\', max_iterations: \'int\' = 2, times_layout: \'str\' = \'aos\', workspace=None)',
    'check_input_feasibility': '(ctx: "\'Context\'", coeffs, times, constraints: \'InputConstraints\', times_layout: \'str\' = \'aos\', want_segments: \'bool\' = True, want_bounds: \'bool\' = True)',
    'check_input_feasibility_host': "(coeffs, times, constraints: 'InputConstraints', times_layout: 'str' = 'aos')",
    'check_input_feasibility_recursive': '(ctx: "\'Context\'", coeffs, times, constraints: \'InputConstraints\', times_layout: \'str\' = \'aos\', want_segments: \'bool\' = True, want_bounds: \'bool\' = True, want_sections: \'bool\' = False)',
    'check_input_feasibility_recursive_host': "(coeffs, times, constraints: 'InputConstraints', times_layout: 'str' = 'aos')",
    'check_half_plane_feasibility': '(ctx: "\'Context\'", coeffs, times, planes, times_layout: \'str\' = \'aos\', want_clearance: \'bool\' = True) -> \'HalfPlaneFeasibilityResult\'',
    'check_half_plane_feasibility_host': "(coeffs, times, planes, times_layout: 'str' = 'aos') -> 'HalfPlaneFeasibilityResult'",
    'check_obstacle_clearance': '(ctx: "\'Context\'", coeffs, times, obstacles, inflation: \'float\' = 0.0, times_layout: \'str\' = \'aos\', want_clearance: \'bool\' = True) -> \'ObstacleClearanceResult\'',
    'check_obstacle_clearance_host': "(coeffs, times, obstacles, inflation: 'float' = 0.0, times_layout: 'str' = 'aos') -> 'ObstacleClearanceResult'",
    'magnitude_soft_cost': "(ctx, coeffs, times, params: 'TimeObjectiveParams', times_layout: 'str' = 'aos')",
    'magnitude_soft_cost_host': "(coeffs, times, params: 'TimeObjectiveParams', times_layout: 'str' = 'aos')",
    'get_input_feasibility_result_name': "(result: 'int') -> 'str'",
    'half_planes': "(points, normals) -> 'np.ndarray'",
    'bounding_box_half_planes': "(center, size) -> 'np.ndarray'",
    'sphere_obstacles': "(centers, radii) -> 'np.ndarray'",
}

# sorted(n for n in dir(m) if not n.startswith("_")) before the calls moved, without the package's submodules (core, buckets, ...):
# dir() lists those of them that something has imported so far, which is no property of the package
EXPORTS = [
    'AxisMinMax', 'Context', 'HalfPlaneFeasibilityResult', 'InputConstraints', 'InputFeasibilityResult', 'MergedRequest',
    'MixedBatchSolver', 'MtgError', 'MultiSolve', 'ObstacleClearanceResult', 'PackedMultiSolve', 'PatternSearchResult', 'Plan',
    'TimeCostKind', 'TimeObjectiveParams', 'TimeObjectiveResult', 'bounding_box_half_planes', 'bounding_boxes',
    'check_half_plane_feasibility', 'check_half_plane_feasibility_host', 'check_input_feasibility',
    'check_input_feasibility_host', 'check_input_feasibility_recursive', 'check_input_feasibility_recursive_host',
    'check_obstacle_clearance', 'check_obstacle_clearance_host', 'ends_full_masks', 'get_input_feasibility_result_name',
    'half_planes', 'library_path', 'magnitude_soft_cost', 'magnitude_soft_cost_host', 'mellinger_cost_and_gradient',
    'minmax_axes', 'minmax_axes_host', 'minmax_magnitude', 'pack_multi_items', 'pattern_search_segment_times',
    'random_waypoint_batch', 'sample_range', 'scale_segment_times_to_meet_constraints', 'solve_linear_batch',
    'sphere_obstacles', 'time_cost_host', 'time_objective']


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signature_is_the_one_before_the_move(name):
    assert str(inspect.signature(getattr(m, name))) == SIGNATURES[name]
    assert getattr(sc, name) is getattr(m, name)


def test_exported_names():
    assert sorted(n for n in dir(m) if not n.startswith("_") and not inspect.ismodule(getattr(m, n))) == EXPORTS
    assert m.core._check is sc._check and m.core.MtgError is m.MtgError
    from mav_trajectory_generation_amd.time_objective_search import magnitude_soft_cost, magnitude_soft_cost_host
    assert magnitude_soft_cost is m.magnitude_soft_cost and magnitude_soft_cost_host is m.magnitude_soft_cost_host


# ---- the six host forms ---------------------------------------------------------------------------------------------------------
B, K, N = 3, 2, 10
CONSTRAINTS = dict(f_min=5.0, f_max=14.0, v_max=3.4, omega_xy_max=0.8, omega_z_max=3.0, omega_z_dot_max=5.0)
# name -> (D, call(coeffs, times, times_layout))
HOST_FORMS = {
    "minmax_axes_host": (3, lambda c, t, lay: m.minmax_axes_host(c, t, 0, 3, times_layout=lay)),
    "check_input_feasibility_host":
        (4, lambda c, t, lay: m.check_input_feasibility_host(c, t, m.InputConstraints(**CONSTRAINTS), times_layout=lay)),
    "check_input_feasibility_recursive_host":
        (4, lambda c, t, lay: m.check_input_feasibility_recursive_host(c, t, m.InputConstraints(**CONSTRAINTS), times_layout=lay)),
    "check_half_plane_feasibility_host":
        (3, lambda c, t, lay: m.check_half_plane_feasibility_host(c, t, m.bounding_box_half_planes([0.1, -0.1, 0.0], [2.6, 2.8, 3.0]),
                                                                  times_layout=lay)),
    "check_obstacle_clearance_host":
        (3, lambda c, t, lay: m.check_obstacle_clearance_host(c, t, m.sphere_obstacles([[0.5, 0.0, 0.2], [-1.0, 1.0, 0.0]], [0.3, 0.5]),
                                                              0.1, times_layout=lay)),
    "magnitude_soft_cost_host":
        (3, lambda c, t, lay: m.magnitude_soft_cost_host(c, t, m.TimeObjectiveParams(constraints=[(1, 2.0), (2, 3.0)]), times_layout=lay)),
}


def same(a, b):
    """Bit-equal arrays (NaN = not computed equals NaN) of one shape and dtype."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name", sorted(HOST_FORMS))
def test_host_forms_share_their_handling(name):
    d, call = HOST_FORMS[name]
    coeffs, times = inputs(B, K, d, N)
    aos = call(coeffs, times, "aos")
    assert type(aos) is type(call(coeffs[:1], times[:1], "aos"))
    assert all(o.shape[0] == B for o in aos)
    soa = call(coeffs, np.ascontiguousarray(times.T), "soa")
    assert type(soa) is type(aos) and len(soa) == len(aos) and all(same(x, y) for x, y in zip(soa, aos))
    frozen = [a.copy() for a in (coeffs, times)]             # (read-only inputs and lists of numbers: converted, not refused)
    for a in frozen:
        a.flags.writeable = False
    assert all(same(x, y) for x, y in zip(call(*frozen, "aos"), aos))
    assert all(same(x, y) for x, y in zip(call(coeffs.tolist(), times.tolist(), "aos"), aos))
    one, single = call(coeffs[:1], times[:1], "aos"), call(coeffs[0], times[0], "aos")
    assert type(single) is type(one) and len(single) == len(one)
    for x, y, full in zip(single, one, aos):
        assert same(x, y[0]) and same(x, full[0]) and np.ndim(x) == np.ndim(y) - 1
    for layout in ("aos", "soa"):
        with pytest.raises(m.MtgError, match="one value per segment"):
            call(coeffs, times.ravel()[:-1], layout)
    with pytest.raises(m.MtgError, match="times_layout"):
        call(coeffs, times, "x")
    with pytest.raises(m.MtgError, match="times_layout"):
        call(coeffs[0], times[0], "AOS")


# ---- the device form's validator, on CPU tensors --------------------------------------------------------------------------------
def test_device_validator_on_cpu_tensors():
    import torch
    ctx = types.SimpleNamespace(device=0)       # (nothing of a context is touched before the inputs are found valid)
    coeffs = torch.zeros((B, K, 3, N), dtype=torch.float64)
    times = torch.ones((B, K), dtype=torch.float64)
    device = sc._SegmentBatch.device
    bad = {
        "float32 coeffs": (coeffs.float(), times, "aos", "must be float64"),
        "float32 times": (coeffs, times.float(), "aos", "must be float64"),
        "3-D coeffs": (coeffs[0], times[0], "aos", r"coeffs must be \[B\]\[K\]\[D\]\[N\]"),
        "non-contiguous coeffs": (coeffs.transpose(2, 3), times, "aos", "must be contiguous"),
        "non-contiguous times": (coeffs, torch.ones((B, 2 * K), dtype=torch.float64)[:, ::2], "aos", "must be contiguous"),
        "times one short": (coeffs, times.reshape(-1)[:B * K - 1], "aos", "one value per segment"),
        "times one short, soa": (coeffs, times.reshape(-1)[:B * K - 1], "soa", "one value per segment"),
        "layout x": (coeffs, times, "x", "times_layout"),
        "soa times shaped [B][K]": (coeffs, times, "soa", "other layout"),
        "aos times shaped [K][B]": (coeffs, times.t().contiguous(), "aos", "other layout"),
    }
    for what, (c, t, layout, message) in bad.items():
        with pytest.raises(m.MtgError, match=message):
            device(ctx, c, t, layout)
            pytest.fail(what)
    for t, layout in ((times, "aos"), (times.t().contiguous(), "soa"), (times.reshape(-1), "aos"), (times.reshape(-1), "soa")):
        with pytest.raises(m.MtgError, match="not a CUDA tensor"):      # everything else is valid
            device(ctx, coeffs, t, layout)
    # a further input (planes, obstacles, a workspace): a batch put together by hand, as the constructor refuses CPU tensors
    batch = sc._SegmentBatch()
    batch.ctx, batch.coeffs, batch.f64 = ctx, coeffs, torch.float64
    planes = torch.zeros((6, 4), dtype=torch.float64)
    assert batch.extra(planes, "planes") is planes
    with pytest.raises(m.MtgError, match="planes must be a float64"):
        batch.extra(planes.float(), "planes")
    with pytest.raises(m.MtgError, match="planes must be contiguous"):
        batch.extra(planes.t(), "planes")
    with pytest.raises(m.MtgError, match="planes must be on the device of coeffs"):
        batch.extra(planes.to("meta"), "planes")
    # and through a public wrapper: the validator runs before anything else does
    with pytest.raises(m.MtgError, match="must be float64"):
        m.check_half_plane_feasibility(ctx, coeffs, times.float(), planes)
    with pytest.raises(m.MtgError, match="not a CUDA tensor"):
        m.sample_range(ctx, coeffs, times, 0.0, 0.1, 4)
