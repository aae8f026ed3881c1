"""Nonlinear time objective with soft constraints, CPU part: the library's host entries mtg_magnitude_soft_cost_host /
mtg_time_cost_host -- the lane code and the cost expressions the device kernels run (csrc/mtg_objective_lane.h) -- on the
REFERENCE's own coefficients against the reference's own callback values (tests/golden/reference_time_objective_*.npz, written by
tests/golden/make_reference_time_objective_golden.py), hand-made polynomials, parameter defaults, argument errors and the ABI
prototypes.  Comparison rules: tests/time_objective_checks.py."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import mav_trajectory_generation_amd as m
from mav_trajectory_generation_amd import _lib as L
from mav_trajectory_generation_amd import TimeObjectiveParams, magnitude_soft_cost_host, time_cost_host  # noqa: F401  (the feature under test)

import time_objective_checks as C

ROOT = C.ROOT
EPS = np.finfo(np.float64).eps


def test_fixture_set_conditions():
    """What the committed set has to hold: the issue's eight cases and the search case, every file no larger than the largest
    feasibility fixture, soft terms from far below one to the cap, no term near the cap (the robustness filter's share is 0)."""
    assert len(C.GOLDEN) == 8 and os.path.exists(C.SEARCH)
    kinds, terms = set(), []
    for path in C.GOLDEN + [C.SEARCH]:
        assert os.path.getsize(path) <= 240565, path
    for name in C.CASE_NAMES:
        z = C.load(name)
        kinds.add((int(z["time_cost_kind"]), int(z["use_soft_constraints"]), int(z["n"]), z["times"].shape[1], z["d_fixed"].shape[1],
                   tuple(z["con_derivative"].tolist()), "d_free" in z.files))
        assert C.near_cap(z, C.HOST_DELTA).mean() <= 0.0, name
        if int(z["use_soft_constraints"]):
            terms.append(C.reference_terms(z)[0].ravel())
    terms = np.concatenate(terms)
    assert terms.min() < 1e-6 and (terms == 1e12).sum() >= 5 and ((terms > 0.1) & (terms < 1e6)).sum() >= 5
    assert (0, 1, 10, 8, 3, (1, 2), False) in kinds and (1, 1, 10, 8, 3, (1, 2), False) in kinds      # squared and Richter time
    assert (0, 0, 10, 8, 3, (1, 2), False) in kinds                                                   # soft constraints off
    assert any(k[3] == 1 for k in kinds)                                                              # K = 1
    assert (0, 1, 10, 16, 4, (1, 2), False) in kinds and (0, 1, 12, 4, 4, (1, 2), False) in kinds     # config-5 shape; N = 12
    assert any(3 in k[5] for k in kinds) and any(k[6] for k in kinds)                                 # a jerk limit; the free form


@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_host_form_on_reference_coefficients(name):
    """mtg_magnitude_soft_cost_host on the reference's OWN coefficients: maxima, every soft term in its exponent, the sum, the
    hard-constraint values; mtg_time_cost_host within 1e-14 relative of the reference's cost_time."""
    z = C.load(name)
    p = C.params_of(z)
    cost, maxima, violations = m.magnitude_soft_cost_host(z["coeffs_ref"], z["times"], p)
    C.check_maxima(maxima, z, C.HOST_DELTA, label=name)
    assert np.array_equal(violations, maxima - z["con_value"])
    ref_terms, expo = C.reference_terms(z)
    if int(z["use_soft_constraints"]):
        # (the restated formula on the reference's maxima reproduces the reference's own sum: the terms are the reference's.  An
        # exponent x carries a few roundings, each eps |x| absolute, which exp turns into that much RELATIVE error of the term)
        allowed = (ref_terms * 4 * EPS * (2.0 + np.abs(expo)) * (ref_terms < float(z["maximum_cost"]))).sum(axis=1) + 4 * EPS * ref_terms.sum(axis=1)
        assert (np.abs(ref_terms.sum(axis=1) - z["components"][:, 2]) <= allowed).all()
        for q in range(len(z["con_value"])):
            term, mx, _ = m.magnitude_soft_cost_host(z["coeffs_ref"], z["times"], C.params_of(z, only=q))
            assert np.array_equal(mx[:, 0], maxima[:, q])
            C.check_term(term, z, q, C.HOST_DELTA, label=name)
        ref_sum, below, above = C.soft_sum_bounds(z, C.HOST_DELTA)
        slack = 8 * EPS * ref_sum          # two sums of at most four terms, rounded
        assert (cost >= ref_sum - below - slack).all() and (cost <= ref_sum + above + slack).all()
    else:
        assert (z["components"][:, 2] == 0.0).all() and (cost == 0.0).all()      # soft term 0, maxima still written
    cost_time = m.time_cost_host(z["times"], p)
    rel = np.abs(cost_time - z["components"][:, 1]) / z["components"][:, 1]
    print(f"{name}: cost_time worst relative difference {rel.max():.2e}")
    assert (rel <= 1e-14).all()


def test_host_form_one_trajectory_and_soa_times():
    z = C.load("n10_k8_d3_squared")
    p = C.params_of(z)
    cost, maxima, _ = m.magnitude_soft_cost_host(z["coeffs_ref"], z["times"], p)
    c1, m1, v1 = m.magnitude_soft_cost_host(z["coeffs_ref"][3], z["times"][3], p)
    assert c1 == cost[3] and np.array_equal(m1, maxima[3]) and v1.shape == (2,)
    c2, m2, _ = m.magnitude_soft_cost_host(z["coeffs_ref"], np.ascontiguousarray(z["times"].T), p, times_layout="soa")
    assert np.array_equal(c2, cost) and np.array_equal(m2, maxima)


def test_hand_made_polynomials():
    """p(t) = (t, 0, 0) then (1 + 2 t + t^2, 0, 0): velocity 1, then 2 + 2 t, peaks at the END of the last segment (4); acceleration
    0 then 2.  exp(100 (4 / 8 - 1)) = exp(-50); a limit of 1 is exceeded four-fold: capped."""
    coeffs = np.zeros((1, 2, 3, 6))
    coeffs[0, 0, 0, 1] = 1.0
    coeffs[0, 1, 0, :3] = (1.0, 2.0, 1.0)
    times = np.array([[1.0, 1.0]])
    p = m.TimeObjectiveParams(constraints=[(1, 8.0), (2, 1.0)])
    cost, maxima, violations = m.magnitude_soft_cost_host(coeffs, times, p)
    assert np.allclose(maxima, [[4.0, 2.0]], rtol=1e-15) and np.allclose(violations, [[-4.0, 1.0]], rtol=1e-15)
    assert cost[0] == math.exp(-50.0) + 1e12
    # an interior maximum: velocity of (3 t^2 - 2 t^3) is 6 t (1 - t), largest 1.5 at t = 0.5
    coeffs = np.zeros((1, 1, 3, 4))
    coeffs[0, 0, 1, 2:] = (3.0, -2.0)
    p = m.TimeObjectiveParams(constraints=[(1, 3.0)], soft_constraint_weight=10.0)
    cost, maxima, _ = m.magnitude_soft_cost_host(coeffs, np.array([[1.0]]), p)
    assert abs(maxima[0, 0] - 1.5) <= 1e-15 and abs(cost[0] - math.exp(-5.0)) <= 1e-15
    # Richter time: penalty * T; squared: penalty * T^2, T summed in segment order
    t = np.array([0.1, 0.2, 0.3])
    assert m.time_cost_host(t, m.TimeObjectiveParams(time_cost_kind=m.TimeCostKind.kRichterTime)) == ((0.1 + 0.2) + 0.3) * 500.0
    assert m.time_cost_host(t, m.TimeObjectiveParams(time_penalty=2.0)) == ((0.1 + 0.2) + 0.3) * ((0.1 + 0.2) + 0.3) * 2.0


def test_parameter_defaults():
    """NonlinearOptimizationParameters' defaults, in Python and as mtg_time_objective_params_init fills them."""
    p = m.TimeObjectiveParams()
    assert (p.time_cost_kind, p.time_penalty, p.use_soft_constraints, p.soft_constraint_weight, p.maximum_cost, p.n_constraints) == \
        (m.TimeCostKind.kSquaredTimeAndConstraints, 500.0, True, 100.0, 1e12, 0)
    c = L.TimeObjectiveParamsC()
    ctypes.memset(ctypes.byref(c), 0xFF, ctypes.sizeof(c))
    L.load().mtg_time_objective_params_init(ctypes.byref(c))
    d = p.to_c()
    for field, _ in L.TimeObjectiveParamsC._fields_[:6]:
        assert getattr(c, field) == getattr(d, field), field
    assert list(c.derivative) == [0, 0, 0, 0] and list(c.value) == [0.0, 0.0, 0.0, 0.0]
    assert [int(k) for k in m.TimeCostKind] == [0, 1, 2, 3, 4]
    p.add_maximum_magnitude_constraint(1, 3.0)
    p.add_maximum_magnitude_constraint(2, 5.0)
    c = p.to_c()
    assert c.n_constraints == 2 and list(c.derivative)[:2] == [1, 2] and list(c.value)[:2] == [3.0, 5.0]


def test_argument_errors():
    coeffs, times = np.zeros((2, 3, 3, 10)), np.ones((2, 3))
    ok = m.TimeObjectiveParams(constraints=[(1, 3.0)])
    m.magnitude_soft_cost_host(coeffs, times, ok)
    with pytest.raises(m.MtgError):
        m.TimeObjectiveParams(constraints=[(0, 3.0)])
    with pytest.raises(m.MtgError):
        m.TimeObjectiveParams(constraints=[(1, -3.0)])
    with pytest.raises(m.MtgError):
        m.TimeObjectiveParams(constraints=[(1, 1.0)] * 5)
    bad = [m.TimeObjectiveParams(constraints=[(5, 3.0)]),                             # N / 2 - 1 = 4 is the highest
           m.TimeObjectiveParams(time_cost_kind=m.TimeCostKind.kMellingerOuterLoop),   # no time term upstream
           m.TimeObjectiveParams(time_cost_kind=7), m.TimeObjectiveParams(time_penalty=float("nan"))]
    for p in bad:
        with pytest.raises(m.MtgError) as e:
            m.magnitude_soft_cost_host(coeffs, times, p)
        assert e.value.code == -1
    with pytest.raises(m.MtgError):
        m.magnitude_soft_cost_host(np.zeros((2, 3, 5, 10)), times, ok)                 # dimension > 4
    with pytest.raises(m.MtgError):
        m.magnitude_soft_cost_host(np.zeros((2, 3, 3, 3)), times, ok)                  # N < 4
    with pytest.raises(m.MtgError):
        m.magnitude_soft_cost_host(coeffs, np.ones((2, 2)), ok)
    with pytest.raises(m.MtgError):
        m.time_cost_host(times, bad[1])
    lib = L.load()
    c = ok.to_c()
    c.n_constraints = 5
    out = np.zeros(2)
    assert lib.mtg_magnitude_soft_cost_host(10, 3, 3, 2, coeffs.ctypes.data, times.ctypes.data, 3, 1, ctypes.byref(c), out.ctypes.data,
                                            None, None) == -1
    c = ok.to_c()
    assert lib.mtg_magnitude_soft_cost_host(10, 3, 3, 2, coeffs.ctypes.data, times.ctypes.data, 1, 1, ctypes.byref(c), out.ctypes.data,
                                            None, None) == -1       # overlapping strides
    assert lib.mtg_magnitude_soft_cost_host(10, 3, 3, 2, None, times.ctypes.data, 3, 1, ctypes.byref(c), out.ctypes.data, None, None) == -1
    assert lib.mtg_magnitude_soft_cost_host(10, 3, 3, 2, coeffs.ctypes.data, times.ctypes.data, 3, 1, ctypes.byref(c), out.ctypes.data,
                                            None, None) == 0        # maxima and violations are optional on the host


def test_abi_prototypes():
    """Every new entry is declared in include/mtg_hip.h, exported by the library and bound with as many arguments as declared; the
    parameter block has the C layout."""
    text = open(os.path.join(ROOT, "include", "mtg_hip.h")).read()
    lib = L.load()
    for name in ("mtg_time_objective_params_init", "mtg_time_objective", "mtg_magnitude_soft_cost", "mtg_magnitude_soft_cost_host",
                 "mtg_time_cost_host"):
        decl = re.search(r"\b(?:int|void) " + name + r"\(([^;]*)\);", text)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(L.EXPORTS[name][1]), name
        assert getattr(lib, name)
    assert re.search(r"#define MTG_MAX_MAGNITUDE_CONSTRAINTS 4\b", text)
    # int32 x2, double x3, int32, int32[4], (4 bytes of padding), double[4]
    assert ctypes.sizeof(L.TimeObjectiveParamsC) == 88 and L.TimeObjectiveParamsC.value.offset == 56
    assert m.time_objective and m.magnitude_soft_cost and m.pattern_search_segment_times and m.TimeObjectiveResult
