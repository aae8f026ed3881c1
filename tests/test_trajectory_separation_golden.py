"""Trajectory-to-trajectory separation check against the reference's own candidates and evaluation
(tests/golden/reference_trajectory_separation_*.npz, make_reference_trajectory_separation_golden.py): the host form here, the
device form in tests/test_gpu_trajectory_separation.py through check_against_fixture."""
import glob
import os

import numpy as np
import pytest

import mav_trajectory_generation_amd as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = {"n10_k8_d3_fast": "reference_feasibility_n10_k8_d3_fast.npz", "n10_k2_d3": "reference_feasibility_n10_k2_d3.npz",
         "n12_k4_d4": "reference_feasibility_n12_k4_d4.npz", "n7_k4_d4": "reference_half_plane_n7_k4_d4.npz"}


def load_case(name):
    """(coeffs, times, the separation golden file): the inputs are the input-feasibility and half-plane fixtures', read from there."""
    src = np.load(os.path.join(GOLDEN, CASES[name]))
    return np.ascontiguousarray(src["coeffs"]), np.ascontiguousarray(src["times"]), np.load(os.path.join(GOLDEN, f"reference_trajectory_separation_{name}.npz"))


def check_against_fixture(name, run):
    """run(coeffs, times, start, pairs, min_separation) -> TrajectorySeparationResult of numpy arrays (both sides the same batch).
    Returns the worst ref - got."""
    coeffs, times, z = load_case(name)
    pairs, msep, robust, scale = z["pairs"], float(z["min_separation"]), z["robust"], z["scale"]
    assert (~robust).sum() <= max(1, len(pairs) // 100)
    assert z["pair_feasible"].sum() >= 5 and (z["pair_feasible"] == 0).sum() >= 5
    r = run(coeffs, times, z["start"], pairs, msep)
    assert np.array_equal(r.pair_feasible[robust], z["pair_feasible"][robust])
    assert np.array_equal(r.first_failing_segment_a[robust], z["first_failing_segment_a"][robust])
    assert np.array_equal(r.first_failing_segment_b[robust], z["first_failing_segment_b"][robust])
    diff = r.pair_separation - (z["distance"] - msep)
    print(f"{name}: got - ref in [{diff.min():.3e}, {diff.max():.3e}], shares of the bounds "
          f"{(diff / (1e-9 * np.maximum(1.0, scale))).max():.2e} / {(-diff / (1e-6 * scale)).max():.2e}")
    # the reference's candidates are values of the same function: its minimum can only be too large -- by what Jenkins-Traub scatters
    # a multiple root at a resting end (the margin tests/helpers.py::assert_extrema_close gives the reference's position minima)
    assert (diff <= 1e-9 * np.maximum(1.0, scale)).all(), float(diff.max())
    assert (-diff <= 1e-6 * scale).all(), float(diff.min())
    # every piece: the per-segment minimum is the smallest of the reference's pieces of that segment, and the counts agree
    ka = coeffs.shape[1]
    count = np.zeros((len(pairs), ka), dtype=np.int32)
    lowest = np.full((len(pairs), ka), np.inf)
    np.add.at(count, (z["piece_pair"], z["piece_a"]), 1)
    np.minimum.at(lowest, (z["piece_pair"], z["piece_a"]), z["piece_distance"])
    assert np.array_equal(r.segment_pieces, count)
    with np.errstate(invalid="ignore"):
        seg = r.segment_separation - (lowest - msep)      # (inf - inf where a segment has no piece)
    has = count > 0
    assert (seg[has] <= 1e-9 * np.maximum(1.0, scale)[:, None].repeat(ka, 1)[has]).all() and (-seg[has] <= 1e-6 * scale[:, None].repeat(ka, 1)[has]).all()
    assert (r.segment_separation[~has] == np.inf).all()
    # the closest piece, where the reference's runner-up is further away than both margins
    for p in range(len(pairs)):
        d = np.sort(z["piece_distance"][z["piece_pair"] == p])
        if len(d) > 1 and d[1] - d[0] > 2e-6 * scale[p]:
            assert (r.pair_closest_segment_a[p], r.pair_closest_segment_b[p]) == (z["closest_segment_a"][p], z["closest_segment_b"][p]), p
    return float((-diff).max())


def test_golden_files_are_complete():
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "reference_trajectory_separation_*.npz"))) == sorted(
        f"reference_trajectory_separation_{c}.npz" for c in CASES)
    for p in glob.glob(os.path.join(GOLDEN, "reference_trajectory_separation_*")):
        assert os.path.getsize(p) <= 300 * 1000, p


@pytest.mark.parametrize("name", CASES)
def test_host_form_against_the_reference(name):
    worst = check_against_fixture(name, lambda c, t, s, pairs, msep: m.check_trajectory_separation_host(c, t, c, t, pairs, msep, start_a=s,
                                                                                                        start_b=s))
    print(f"{name}: worst ref - got {worst:.3e}")
