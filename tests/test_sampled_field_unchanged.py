"""The sampled distance-field check after its lookup was split into a voxel-coordinate part and a value part (for the certified
check, csrc/mtg_certify_lane.h): mtg_check_distance_field_host is bit for bit what it was.  The expected outputs
(tests/golden/sampled_field_parent_host.npz) were written by the host form of the commit BEFORE the split -- its
mtg_field_host.cpp and headers compiled on their own -- on two fixture cases with the fields of tests/test_distance_field.py, never
by the code under test."""
import os

import numpy as np
import pytest

import mav_trajectory_generation_amd as m
from test_distance_field import DT, H, INFLATION, field_case

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampled_field_parent_host.npz")
MODES = {"tri_out0": (0.0, "trilinear"), "tri_outinf": (np.inf, "trilinear"), "near_out0": (0.0, "nearest")}
FIELDS = ("trajectory_feasible", "first_failing_segment", "segment_clearance", "segment_closest_sample", "segment_first_failing_sample",
          "segment_samples", "trajectory_clearance")


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", ["n10_k8_d3_fast", "n7_k4_d4"])
def test_host_form_is_bit_identical_to_the_parent(name, mode):
    z = np.load(GOLDEN)
    coeffs, times, grid, origin = field_case(name)
    outside, interpolation = MODES[mode]
    r = m.check_distance_field_host(coeffs, times, m.DistanceField(grid, origin, H, outside, interpolation), DT, inflation=INFLATION)
    for f in FIELDS:
        want, got = z[f"{name}/{mode}/{f}"], getattr(r, f)
        assert want.dtype == got.dtype and want.shape == got.shape
        assert want.tobytes() == got.tobytes(), f                      # bits, not values: a NaN's payload and a zero's sign too


def test_the_lookup_is_still_one_function_of_two_parts():
    src = open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "mav_trajectory_generation_amd", "csrc", "mtg_field_lane.h")).read()
    assert "voxel_coordinates(g, p, u);" in src and "return lookup_voxel(g, u);" in src
