"""What the CPU and the GPU tests of the nonlinear time objective share: the fixtures of
tests/golden/make_reference_time_objective_golden.py and the comparison rules.

Rules (none of them tuned to what the code gives):
  * maxima of velocity / acceleration: |got - ref| <= delta * ref; jerk and above: -delta <= (got - ref) / ref <= delta_up
    (the rule of helpers.assert_extrema_close: higher derivatives often peak at the trajectory ends, where the reference's
    Jenkins-Traub scatters a multiple root and evaluates next to it, so ours may be LARGER by up to 1e-6);
  * an uncapped soft term exp(w (max / limit - 1)) is compared in its exponent: d ln(term) = w d(max) / limit, so a maximum good
    to delta relative gives |ln got - ln ref| <= w (max_ref / limit) delta -- derived from the maxima tolerance, nothing else;
  * terms that both sides cap are equal exactly; a term whose reference exponent lies within that band of ln(maximum_cost) could be
    capped on one side only and is not compared -- the committed fixtures hold no such term (asserted).
"""
import glob
import math
import os

import numpy as np

import mav_trajectory_generation_amd as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(p for p in glob.glob(os.path.join(ROOT, "tests", "golden", "reference_time_objective_*.npz"))
                if not p.endswith("_search.npz"))
SEARCH = os.path.join(ROOT, "tests", "golden", "reference_time_objective_search.npz")
CASE_NAMES = [os.path.basename(p)[len("reference_time_objective_"):-len(".npz")] for p in GOLDEN]
HOST_DELTA = 1e-9       # the bound of helpers.assert_extrema_close on maxima of velocity / acceleration
JERK_DELTA_UP = 1e-6    # ... and its one-sided allowance above the reference for the other derivatives


def load(name):
    return np.load(os.path.join(ROOT, "tests", "golden", f"reference_time_objective_{name}.npz"))


def params_of(z, only=None):
    """TimeObjectiveParams of a fixture; only = index of the one constraint to keep (a soft cost of one term)."""
    cons = list(zip(z["con_derivative"].tolist(), z["con_value"].tolist()))
    if only is not None:
        cons = [cons[only]]
    return m.TimeObjectiveParams(time_cost_kind=int(z["time_cost_kind"]), time_penalty=float(z["time_penalty"]),
                                 use_soft_constraints=bool(int(z["use_soft_constraints"])),
                                 soft_constraint_weight=float(z["soft_constraint_weight"]), maximum_cost=float(z["maximum_cost"]),
                                 constraints=cons)


def deltas(derivative, delta, extra_up=0.0):
    """(downwards, upwards) relative tolerance of a maximum of this derivative."""
    return (delta, delta) if derivative in (1, 2) else (delta, JERK_DELTA_UP + extra_up)


def check_maxima(got, z, delta, extra_up=0.0, label=""):
    ref = z["maxima"]
    assert got.shape == ref.shape
    for q, der in enumerate(z["con_derivative"].tolist()):
        lo, up = deltas(der, delta, extra_up)
        rel = (got[:, q] - ref[:, q]) / ref[:, q]
        print(f"{label} maxima of derivative {der}: (got - ref) / ref in [{rel.min():.2e}, {rel.max():.2e}], allowed [-{lo:.0e}, {up:.0e}]")
        assert (rel >= -lo).all() and (rel <= up).all(), (label, der, rel.min(), rel.max())


def reference_terms(z):
    """(terms [B][C] as the reference's formula gives them from ITS maxima, exponents [B][C])."""
    w, cap = float(z["soft_constraint_weight"]), float(z["maximum_cost"])
    expo = (z["maxima"] - z["con_value"]) / z["con_value"] * w       # in the reference's order of operations (:780-785)
    with np.errstate(over="ignore"):
        return np.minimum(cap, np.exp(expo)), expo


def bands(z, delta, extra_up=0.0):
    """[B][C][2]: how far below / above the reference's a term's exponent may lie."""
    w = float(z["soft_constraint_weight"])
    out = np.zeros(z["maxima"].shape + (2,))
    for q, der in enumerate(z["con_derivative"].tolist()):
        lo, up = deltas(der, delta, extra_up)
        out[:, q, 0] = w * (z["maxima"][:, q] / z["con_value"][q]) * lo
        out[:, q, 1] = w * (z["maxima"][:, q] / z["con_value"][q]) * up
    return out


def near_cap(z, delta, extra_up=0.0):
    _, expo = reference_terms(z)
    band = bands(z, delta, extra_up).max(axis=-1)
    return np.abs(expo - math.log(float(z["maximum_cost"]))) <= band


def check_term(got, z, q, delta, extra_up=0.0, label=""):
    """One soft term per trajectory (a soft cost evaluated with constraint q alone) against the reference's."""
    cap = float(z["maximum_cost"])
    ref, expo = reference_terms(z)
    ref, expo = ref[:, q], expo[:, q]
    band = bands(z, delta, extra_up)[:, q]
    skip = near_cap(z, delta, extra_up)[:, q]
    assert skip.mean() <= 0.0, (label, q, skip.mean())       # the robustness filter: no such term on the committed fixtures
    capped = expo > math.log(cap)
    assert np.array_equal(got[capped], ref[capped]) and (got[capped] == cap).all(), (label, q)
    assert (got[~capped] < cap).all()
    d = np.log(got[~capped]) - expo[~capped]
    print(f"{label} soft term {q}: {int(capped.sum())} capped, ln got - ln ref in [{d.min() if d.size else 0.0:.2e}, "
          f"{d.max() if d.size else 0.0:.2e}], tightest band {band[~capped].min() if d.size else 0.0:.2e}")
    assert (d >= -band[~capped, 0]).all() and (d <= band[~capped, 1]).all(), (label, q, d.min(), d.max())


def soft_sum_bounds(z, delta, extra_up=0.0):
    """(reference sum [B], how far below [B], how far above [B]) a sum of soft terms may lie when every uncapped term obeys the
    exponent rule and the capped ones are exact: sum_q ref_q (exp(+-band_q) - 1)."""
    ref, expo = reference_terms(z)
    band = bands(z, delta, extra_up)
    capped = expo > math.log(float(z["maximum_cost"]))
    below = np.where(capped, 0.0, ref * -np.expm1(-band[..., 0])).sum(axis=1)
    above = np.where(capped, 0.0, ref * np.expm1(band[..., 1])).sum(axis=1)
    return ref.sum(axis=1), below, above
