"""mav_trajectory_generation_amd -- MI355X-native batched PolynomialOptimization<N>::solveLinear().

Host-side plumbing only: the compute path is the hand-written HIP library
csrc/libmtg_hip.so (C ABI in include/mtg_hip.h).  There is NO CPU fallback: importing the
solver entry points without the built library, or calling them without a GPU, raises.
"""
from .core import Context, Plan, MtgError, MultiSolve, solve_linear_batch, library_path  # noqa: F401
from .core import pack_multi_items, PackedMultiSolve  # noqa: F401
from .segment_checks import sample_range, minmax_magnitude, scale_segment_times_to_meet_constraints  # noqa: F401
from .segment_checks import InputConstraints, InputFeasibilityResult, check_input_feasibility, check_input_feasibility_host  # noqa: F401
from .segment_checks import get_input_feasibility_result_name  # noqa: F401
from .segment_checks import check_input_feasibility_recursive, check_input_feasibility_recursive_host  # noqa: F401
from .segment_checks import half_planes, bounding_box_half_planes, check_half_plane_feasibility  # noqa: F401
from .segment_checks import check_half_plane_feasibility_host, HalfPlaneFeasibilityResult  # noqa: F401
from .segment_checks import sphere_obstacles, check_obstacle_clearance, check_obstacle_clearance_host, ObstacleClearanceResult  # noqa: F401
from .segment_checks import AxisMinMax, minmax_axes, minmax_axes_host, bounding_boxes  # noqa: F401
from .workload import ends_full_masks, random_waypoint_batch  # noqa: F401
from .buckets import MergedRequest, MixedBatchSolver  # noqa: F401
from .time_gradient import mellinger_cost_and_gradient  # noqa: F401
from .time_objective_search import TimeObjectiveParams, TimeObjectiveResult, TimeCostKind, time_objective  # noqa: F401
from .time_objective_search import magnitude_soft_cost, magnitude_soft_cost_host, pattern_search_segment_times  # noqa: F401
from .time_objective_search import PatternSearchResult, time_cost_host  # noqa: F401


# The keep-out zone check: mav_trajectory_generation_amd.check_keep_out_zones and its companions resolve here on first use
# (PEP 562).  They are not bound at import: tests/test_segment_batch.py pins dir() of the package to the list it had when the
# per-segment calls moved to segment_checks.py.
_KEEP_OUT = ("keep_out_boxes", "check_keep_out_zones", "check_keep_out_zones_host", "KeepOutResult")
# (the distance-field check likewise)
_DISTANCE_FIELD = ("DistanceField", "DistanceFieldResult", "check_distance_field", "check_distance_field_host")
# (and the certified distance-field check)
_CERTIFIED_FIELD = ("CertifiedFieldResult", "certify_distance_field", "certify_distance_field_host")
# (and the trajectory-to-trajectory separation check)
_SEPARATION = ("TrajectorySeparationResult", "check_trajectory_separation", "check_trajectory_separation_host", "all_pairs")
# (and the distance-field collision cost and gradient)
_COLLISION_COST = ("CollisionCostResult", "collision_cost", "collision_cost_host")

# (and the gradient with respect to the free derivatives: Plan.free_gradient is a method; the host form lives in core.py)
_FREE_GRADIENT = ("free_gradient_host",)


def __getattr__(name):
    if name in _FREE_GRADIENT:
        from . import core
        return getattr(core, name)
    if name in _KEEP_OUT or name in _DISTANCE_FIELD or name in _CERTIFIED_FIELD or name in _SEPARATION or name in _COLLISION_COST:
        from . import segment_checks
        return getattr(segment_checks, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
