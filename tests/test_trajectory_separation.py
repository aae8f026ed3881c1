"""Trajectory-to-trajectory separation check, host form (mtg_check_trajectory_separation_host: the lane code of
csrc/mtg_separation_lane.h compiled by g++; no device): against an independent exact reference
(tests/trajectory_separation_ref.py), identities that need no reference, independence of pruning (tests/separation_emu.cpp),
the rules for degenerate pairs, layouts and shapes."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import mav_trajectory_generation_amd as m
from mav_trajectory_generation_amd import _lib as L
import trajectory_separation_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mav_trajectory_generation_amd", "csrc")


def host(z, **kw):
    args = dict(start_a=z["start_a"], start_b=z["start_b"])
    args.update(kw)
    return m.check_trajectory_separation_host(z["coeffs_a"], z["times_a"], z["coeffs_b"], z["times_b"], z["pairs"], z["min_separation"],
                                              **args)


def runner_up_gap(values):
    v = sorted(values)
    return v[1] - v[0] if len(v) > 1 else R.LD(np.inf)


def compare_with_reference(z, r, pieces=None, scale=None):
    """Values within 1e-9 max(1, scale); piece counts equal; verdicts and first-failure indices equal on pairs whose reference verdict
    and indices do not change under min_separation (1 +- 1e-6); closest-segment indices equal where the reference's runner-up is
    further away than twice the bound.  At most max(1, P // 100) pairs, and at most 1 %, may be left out.  Returns the largest share
    of the value bound."""
    pieces = z["pieces"] if pieces is None else pieces
    scale = z["scale"] if scale is None else scale
    msep, ka, npairs = z["min_separation"], z["coeffs_a"].shape[1], len(z["pairs"])
    share, left_out = 0.0, 0
    for p in range(npairs):
        (a, b), bound = z["pairs"][p], 1e-9 * max(1.0, scale[p])
        f = R.fold(pieces[p], ka, msep)
        assert np.array_equal(r.segment_pieces[p], f["segment_pieces"]), p
        if not pieces[p]:
            assert r.pair_feasible[p] == 1 and r.pair_separation[p] == np.inf and np.isnan(r.pair_closest_time[p]), p
            assert (r.first_failing_segment_a[p], r.first_failing_segment_b[p]) == (-1, -1), p
            assert (r.pair_closest_segment_a[p], r.pair_closest_segment_b[p]) == (-1, -1), p
            assert (r.segment_separation[p] == np.inf).all() and np.isnan(r.segment_closest_time[p]).all(), p
            assert (r.segment_closest_segment_b[p] == -1).all(), p
            continue
        err = float(abs(R.LD(r.pair_separation[p]) - (f["distance"] - R.LD(msep))))
        assert err <= bound, (p, err, bound)
        share = max(share, err / bound)
        skip = False
        for i in range(ka):
            if f["segment_pieces"][i] == 0:
                assert r.segment_separation[p, i] == np.inf and np.isnan(r.segment_closest_time[p, i]), (p, i)
                assert r.segment_closest_segment_b[p, i] == -1, (p, i)
                continue
            err = float(abs(R.LD(r.segment_separation[p, i]) - (f["segment_distance"][i] - R.LD(msep))))
            assert err <= bound, (p, i, err, bound)
            share = max(share, err / bound)
            # the reported time is a time at which the two ORIGINAL curves are that far apart
            t, j = r.segment_closest_time[p, i], r.segment_closest_segment_b[p, i]
            ea, eb = R.breakpoints(z["times_a"][a], z["start_a"][a]), R.breakpoints(z["times_b"][b], z["start_b"][b])
            assert 0 <= j < len(eb) - 1 and max(ea[i], eb[j]) <= t <= min(ea[i + 1], eb[j + 1]), (p, i, j, t)
            ta, tb = R.LD(t) - R.LD(ea[i]), R.LD(t) - R.LD(eb[j])
            d = R.distance(z["coeffs_a"][a, i], ta, z["coeffs_b"][b, j], tb, [0.0])[0]
            assert float(abs(d - R.LD(msep) - R.LD(r.segment_separation[p, i]))) <= bound, (p, i)
            if runner_up_gap([q[4] for q in pieces[p] if q[0] == i]) > 2 * bound:
                assert j == f["segment_b_of"][i], (p, i)
            else:
                skip = True
        lo, hi = R.fold(pieces[p], ka, msep * (1 - 1e-6)), R.fold(pieces[p], ka, msep * (1 + 1e-6))
        if (lo["feasible"], lo["first"]) == (f["feasible"], f["first"]) == (hi["feasible"], hi["first"]):
            assert r.pair_feasible[p] == f["feasible"], p
            assert (r.first_failing_segment_a[p], r.first_failing_segment_b[p]) == f["first"], p
        else:
            skip = True
        if f["runner_up"] - f["distance"] > 2 * bound:
            assert (r.pair_closest_segment_a[p], r.pair_closest_segment_b[p]) == (f["segment_a"], f["segment_b"]), p
            i = f["segment_a"]
            assert r.pair_closest_time[p] == r.segment_closest_time[p, i], p
        else:
            skip = True
        left_out += skip
    assert left_out <= max(1, npairs // 100) and left_out <= max(1.0, 0.01 * npairs), left_out
    return share


@pytest.mark.parametrize("n,d,family", R.CASES)
def test_host_form_against_the_independent_reference(n, d, family):
    """Largest measured share of the bound 1e-9 max(1, scale) over the 72 cases: see DESIGN.md section 4.16."""
    z = R.reference(n, d, family)
    r = host(z)
    share = compare_with_reference(z, r)
    print(f"n{n} d{d} {family}: largest share of the bound {share:.2e}")
    feas = r.pair_feasible
    if family == "far":
        assert feas.all()
    if family == "crossing":
        assert not feas.all() and (r.pair_separation <= -z["min_separation"] + 1e-9 * z["scale"]).any()


@pytest.mark.parametrize("n,d,family", [(10, 3, "random"), (12, 4, "crossing"), (5, 3, "far"), (1, 3, "random"), (7, 4, "random")])
def test_the_independent_reference_misses_nothing(n, d, family):
    z = R.reference(n, d, family)
    for p, (a, b) in enumerate(z["pairs"]):
        grid = R.grid_min(z["coeffs_a"][a], z["times_a"][a], z["start_a"][a], z["coeffs_b"][b], z["times_b"][b], z["start_b"][b])
        best = min([q[4] for q in z["pieces"][p]], default=R.LD(np.inf))
        assert float(best) <= grid + 1e-9 * max(1.0, z["scale"][p]), (p, float(best), grid)


@pytest.mark.parametrize("ka,kb", [(1, 5), (5, 1), (3, 8), (1, 1), (6, 2)])
def test_segment_counts_differ(ka, kb):
    z = R.make_inputs(10, 3, "random", ka=ka, kb=kb)
    z["pieces"] = R.reference_of(z)
    z["scale"] = R.scale_of(z["coeffs_a"], z["times_a"], z["coeffs_b"], z["times_b"], z["pairs"], z["min_separation"])
    r = host(z)
    assert r.segment_separation.shape == (R.P, ka)
    print(f"ka{ka} kb{kb}: largest share of the bound {compare_with_reference(z, r):.2e}")


def breakpoint_case(start_b):
    """Two trajectories of A (3 segments) and one of B (2 segments) with times that are exact in binary, B started at start_b."""
    z = R.make_inputs(8, 3, "random", ka=3, kb=2, ba=2, bb=1, n_pairs=2)
    z["times_a"] = np.array([[1.0, 0.5, 1.25], [0.75, 0.25, 1.0]])
    z["times_b"] = np.array([[0.75, 1.5]])
    z["start_a"], z["start_b"] = np.zeros(2), np.array([start_b])
    z["pairs"] = np.array([[0, 0], [1, 0]], dtype=np.int32)
    z["pieces"] = R.reference_of(z)
    z["scale"] = R.scale_of(z["coeffs_a"], z["times_a"], z["coeffs_b"], z["times_b"], z["pairs"], z["min_separation"])
    return z


def test_start_offsets_and_breakpoints():
    # the window is empty; the window touches at an instant (B starts exactly where A's trajectory 0 ends)
    for start_b in (100.0, 2.75):
        z = breakpoint_case(start_b)
        assert z["pieces"][0] == []
        r = host(z)
        compare_with_reference(z, r)
        assert r.pair_feasible[0] == 1 and r.pair_separation[0] == np.inf and (r.segment_pieces[0] == 0).all()
    # a breakpoint of B equals a breakpoint of A exactly: three pieces, not four
    z = breakpoint_case(0.25)
    assert R.breakpoints(z["times_b"][0], 0.25)[1] == R.breakpoints(z["times_a"][0], 0.0)[1] == 1.0
    r = host(z)
    compare_with_reference(z, r)
    assert r.segment_pieces[0].tolist() == [1, 1, 1]
    # ... and falls 1 ulp beside it: segment 0 of B reaches 1 ulp into segment 1 of A, a piece of its own
    beside = float(np.nextafter(1.0, 2.0)) - 0.75
    z = breakpoint_case(beside)
    assert R.breakpoints(z["times_b"][0], beside)[1] == np.nextafter(1.0, 2.0)
    r = host(z)
    compare_with_reference(z, r)
    assert r.segment_pieces[0].tolist() == [1, 2, 1]
    assert [(q[0], q[1]) for q in z["pieces"][0]] == [(0, 0), (1, 0), (1, 1), (2, 1)]


def test_both_times_layouts():
    z = R.reference(10, 3, "random")
    r = host(z)
    soa = m.check_trajectory_separation_host(z["coeffs_a"], np.ascontiguousarray(z["times_a"].T), z["coeffs_b"],
                                             np.ascontiguousarray(z["times_b"].T), z["pairs"], z["min_separation"], start_a=z["start_a"],
                                             start_b=z["start_b"], times_layout="soa")
    for x, y in zip(r, soa):
        assert np.array_equal(x, y, equal_nan=True)
    # no starts: both sides start at 0
    zero = host(z, start_a=None, start_b=None)
    given = host(z, start_a=np.zeros(R.BA), start_b=np.zeros(R.BB))
    for x, y in zip(zero, given):
        assert np.array_equal(x, y, equal_nan=True)
    # without the closest approach the first four outputs are the same
    few = host(z, want_closest=False)
    assert all(x is None for x in few[4:])
    for x, y in zip(few[:4], r[:4]):
        assert np.array_equal(x, y, equal_nan=True)


def test_identity_a_constant_point_is_a_sphere_of_radius_zero():
    for n, d in ((10, 3), (7, 4), (4, 3)):
        z = R.make_inputs(n, d, "random", ka=5, kb=5, ba=9, bb=9, n_pairs=9)
        rng = np.random.default_rng(n)
        points = rng.uniform(-2.0, 2.0, size=(9, 3))
        cb = np.zeros_like(z["coeffs_b"])
        cb[:, :, :3, 0] = points[:, None, :]
        pairs = np.stack([np.arange(9), np.arange(9)], axis=1).astype(np.int32)
        msep = 1.25
        r = m.check_trajectory_separation_host(z["coeffs_a"], z["times_a"], cb, z["times_a"], pairs, msep)
        obstacles = np.concatenate([points, np.zeros((9, 1))], axis=1)[:, None, :]
        o = m.check_obstacle_clearance_host(z["coeffs_a"], z["times_a"], obstacles, inflation=msep)
        bound = 1e-9 * np.maximum(1.0, R.scale_of(z["coeffs_a"], z["times_a"], cb, z["times_a"], pairs, msep))
        assert (np.abs(r.pair_separation - o.trajectory_clearance) <= bound).all()
        assert (np.abs(r.segment_separation - o.segment_clearance) <= bound[:, None]).all()
        assert (r.segment_pieces == 1).all() and (r.segment_closest_segment_b == np.arange(5)).all()
        robust = (np.abs(o.segment_clearance) > 2 * bound[:, None]).all(axis=1)
        assert robust.sum() >= 8
        assert np.array_equal(r.pair_feasible[robust], o.trajectory_feasible[robust])
        assert np.array_equal(r.first_failing_segment_a[robust], o.first_failing_segment[robust])
        assert np.array_equal(r.first_failing_segment_b[robust], o.first_failing_segment[robust])
        assert not r.pair_feasible.all() and r.pair_feasible.any()


@pytest.mark.parametrize("n,d,family", [(10, 3, "random"), (12, 4, "crossing"), (5, 3, "far"), (3, 4, "random")])
def test_identity_b_swapping_the_sides(n, d, family):
    z = R.reference(n, d, family)
    r = host(z)
    s = m.check_trajectory_separation_host(z["coeffs_b"], z["times_b"], z["coeffs_a"], z["times_a"], np.ascontiguousarray(z["pairs"][:, ::-1]),
                                           z["min_separation"], start_a=z["start_b"], start_b=z["start_a"])
    bound = 1e-9 * np.maximum(1.0, z["scale"])
    assert np.array_equal(r.pair_feasible, s.pair_feasible)
    assert np.array_equal(r.first_failing_segment_a, s.first_failing_segment_b) and np.array_equal(r.first_failing_segment_b, s.first_failing_segment_a)
    assert np.array_equal(r.pair_closest_segment_a, s.pair_closest_segment_b) and np.array_equal(r.pair_closest_segment_b, s.pair_closest_segment_a)
    assert (np.abs(r.pair_separation - s.pair_separation) <= bound).all()
    assert (np.abs(r.pair_closest_time - s.pair_closest_time) <= bound).all()


def test_identity_c_a_trajectory_against_itself():
    z = R.reference(10, 3, "random")
    pairs = np.stack([np.arange(R.BA), np.arange(R.BA)], axis=1).astype(np.int32)
    for msep in (0.0, 0.75):
        r = m.check_trajectory_separation_host(z["coeffs_a"], z["times_a"], z["coeffs_a"], z["times_a"], pairs, msep, start_a=z["start_a"],
                                               start_b=z["start_a"])
        assert (r.pair_separation == -msep).all() and (r.segment_separation == -msep).all() and not r.pair_feasible.any()
        assert (r.first_failing_segment_a == 0).all() and (r.first_failing_segment_b == 0).all()
        assert (r.pair_closest_segment_a == 0).all() and (r.pair_closest_segment_b == 0).all()
        assert np.array_equal(r.pair_closest_time, z["start_a"])


def test_identity_d_appended_pairs_change_nothing():
    z = R.reference(10, 3, "random")
    r = host(z)
    away = z["coeffs_b"].copy()
    away[:, :, 0, 0] += 60.0
    cb = np.concatenate([z["coeffs_b"], away])
    tb = np.concatenate([z["times_b"], z["times_b"]])
    sb = np.concatenate([z["start_b"], z["start_b"]])
    more = np.concatenate([z["pairs"], np.stack([np.arange(6) % R.BA, R.BB + np.arange(6)], axis=1).astype(np.int32)])
    s = m.check_trajectory_separation_host(z["coeffs_a"], z["times_a"], cb, tb, more, z["min_separation"], start_a=z["start_a"], start_b=sb)
    for x, y in zip(r, s):
        assert np.array_equal(x, y[:R.P], equal_nan=True)
    assert s.pair_feasible[R.P:].all() and (s.pair_separation[R.P:] > 20.0).all()


def test_nan_negative_time_and_non_finite_start():
    z = R.reference(10, 3, "random")
    clean = host(z)
    a0, b0 = z["pairs"][0]
    touched = lambda side, index: z["pairs"][:, side] == index
    # a NaN coefficient: the pieces it enters are NaN, the pair's separation is NaN and the pair fails
    ca = z["coeffs_a"].copy()
    ca[a0, 2, 1, 3] = np.nan
    r = host(dict(z, coeffs_a=ca))
    hit = touched(0, a0)
    assert np.isnan(r.pair_separation[hit]).all() and not r.pair_feasible[hit].any()
    had = clean.segment_pieces[hit][:, 2] > 0
    assert had.any() and np.isnan(r.segment_separation[hit][had, 2]).all()
    assert (r.first_failing_segment_a[hit][had] <= 2).all() and (r.first_failing_segment_a[hit][had] >= 0).all()
    for x, y in zip(r, clean):
        assert np.array_equal(x[~hit], y[~hit], equal_nan=True)
    # unusable times and starts, on either side: the pair is infeasible, NaN, without indices or pieces
    for key, index, side, value in (("times_a", (a0, 1), 0, -0.5), ("times_a", (a0, 4), 0, np.inf), ("times_b", (b0, 0), 1, np.nan),
                                    ("start_a", a0, 0, np.inf), ("start_b", b0, 1, np.nan)):
        x = z[key].copy()
        x[index] = value
        r = host(dict(z, **{key: x}))
        hit = touched(side, a0 if side == 0 else b0)
        assert not r.pair_feasible[hit].any() and np.isnan(r.pair_separation[hit]).all() and np.isnan(r.pair_closest_time[hit]).all(), key
        for out in (r.first_failing_segment_a, r.first_failing_segment_b, r.pair_closest_segment_a, r.pair_closest_segment_b,
                    r.segment_closest_segment_b):
            assert (out[hit] == -1).all(), key
        assert np.isnan(r.segment_separation[hit]).all() and np.isnan(r.segment_closest_time[hit]).all() and (r.segment_pieces[hit] == 0).all()
        for u, v in zip(r, clean):
            assert np.array_equal(u[~hit], v[~hit], equal_nan=True)
    # a segment of time 0 is allowed: it makes no piece
    ta = z["times_a"].copy()
    ta[a0, 1] = 0.0
    r = host(dict(z, times_a=ta))
    assert (r.segment_pieces[touched(0, a0)][:, 1] == 0).all() and not np.isnan(r.pair_separation).any()


def test_pair_index_out_of_range_raises():
    z = R.reference(10, 3, "random")
    for bad in ([R.BA, 0], [-1, 0], [0, R.BB], [0, -1]):
        pairs = z["pairs"].copy()
        pairs[5] = bad
        with pytest.raises(m.MtgError):
            host(dict(z, pairs=pairs))
    assert len(host(dict(z, pairs=np.zeros((0, 2), dtype=np.int32))).pair_feasible) == 0


def test_all_pairs_helper():
    assert m.all_pairs(4).tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    p = m.all_pairs(16)
    assert p.shape == (120, 2) and p.dtype == np.int32 and p.flags.c_contiguous and (p[:, 0] < p[:, 1]).all()
    assert m.all_pairs(1).shape == (0, 2)


def test_outputs_are_written_in_full_and_not_beyond():
    lib = L.load()
    z = R.reference(12, 4, "crossing")
    r = host(z)
    ka, kb = z["coeffs_a"].shape[1], z["coeffs_b"].shape[1]
    pad = 3
    i32 = lambda size: np.full((size + 2 * pad,), -77, dtype=np.int32)
    f64 = lambda size: np.full((size + 2 * pad,), -77.5)
    bufs = [i32(R.P), i32(R.P), i32(R.P), f64(R.P), f64(R.P), i32(R.P), i32(R.P), f64(R.P * ka), f64(R.P * ka), i32(R.P * ka), i32(R.P * ka)]
    ptr = lambda a: a.ctypes.data + pad * a.itemsize
    sa, sb = np.ascontiguousarray(z["start_a"]), np.ascontiguousarray(z["start_b"])
    head = (12, 4, ka, R.BA, z["coeffs_a"].ctypes.data, z["times_a"].ctypes.data, ka, 1, sa.ctypes.data, kb, R.BB, z["coeffs_b"].ctypes.data,
            z["times_b"].ctypes.data, kb, 1, sb.ctypes.data, R.P, z["pairs"].ctypes.data, z["min_separation"])
    assert lib.mtg_check_trajectory_separation_host(*head, *[ptr(a) for a in bufs]) == 0
    for a, want in zip(bufs, r):
        assert (a[:pad] == a.dtype.type(-77 if a.dtype == np.int32 else -77.5)).all() and (a[-pad:] == a[:pad]).all()
        assert np.array_equal(a[pad:-pad], np.asarray(want).ravel(), equal_nan=True)
    feas = np.empty((R.P,), dtype=np.int32)
    assert lib.mtg_check_trajectory_separation_host(*head, feas.ctypes.data, *([None] * 10)) == 0
    assert np.array_equal(feas, r.pair_feasible)


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "mtg_hip.h")).read()
    for name in ("mtg_check_trajectory_separation", "mtg_check_trajectory_separation_host"):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(L.EXPORTS[name][1]), name
    assert len(L.EXPORTS["mtg_check_trajectory_separation"][1]) == 31 and len(L.EXPORTS["mtg_check_trajectory_separation_host"][1]) == 30


# ---- the lane with its test knobs: pruning changes nothing, and it does prune -------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    so, src = os.path.join(ROOT, "tests", "libmtg_separation_emu.so"), os.path.join(ROOT, "tests", "separation_emu.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in ("mtg_separation_lane.h", "mtg_obstacle_lane.h", "mtg_segment_lane.h", "mtg_extrema_lane.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    p = ctypes.c_void_p
    lib.separation_emu_lane.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, p, p, ctypes.c_double, ctypes.c_int, p, p, ctypes.c_double,
                                        ctypes.c_int, ctypes.c_double, ctypes.c_int, p, p]
    return lib


def lanes(emu, z, prune):
    """[P][Ka] rows (separation, time) and (segment_b, failing_a, failing_b, pieces, invalid, searches) of every lane."""
    n, d, ka, kb = z["coeffs_a"].shape[3], z["coeffs_a"].shape[2], z["coeffs_a"].shape[1], z["coeffs_b"].shape[1]
    f, i = np.zeros((len(z["pairs"]), ka, 2)), np.zeros((len(z["pairs"]), ka, 6), dtype=np.int32)
    for p, (a, b) in enumerate(z["pairs"]):
        ca, ta, cb, tb = (np.ascontiguousarray(x) for x in (z["coeffs_a"][a], z["times_a"][a], z["coeffs_b"][b], z["times_b"][b]))
        for s in range(ka):
            assert emu.separation_emu_lane(n, d, ka, ca.ctypes.data, ta.ctypes.data, float(z["start_a"][a]), kb, cb.ctypes.data, tb.ctypes.data,
                                           float(z["start_b"][b]), s, z["min_separation"], int(prune), f[p, s].ctypes.data, i[p, s].ctypes.data) == 0
    return f, i


@pytest.mark.parametrize("n,d", [(4, 3), (5, 3), (7, 4), (8, 3), (10, 3), (12, 4)])
def test_pruning_changes_no_output_and_does_prune(emu, n, d):
    searched = {}
    for family in R.FAMILIES:
        z = R.reference(n, d, family)
        f0, i0 = lanes(emu, z, False)
        f1, i1 = lanes(emu, z, True)
        assert f0.tobytes() == f1.tobytes() and np.array_equal(i0[:, :, :5], i1[:, :, :5]), family
        assert np.array_equal(i0[:, :, 5], i0[:, :, 3])                    # without pruning every piece is searched
        assert (i1[:, :, 5] <= i1[:, :, 3]).all()
        searched[family] = (int(i1[:, :, 5].sum()), int(i1[:, :, 3].sum()))
        # ... and the library's host form is this lane
        r = host(z)
        assert r.segment_separation.tobytes() == np.ascontiguousarray(f1[:, :, 0]).tobytes()
        assert np.array_equal(r.segment_pieces, i1[:, :, 3]) and np.array_equal(r.segment_closest_segment_b, i1[:, :, 0])
    print(f"n{n} d{d}: searches / pieces {searched}")
    assert searched["far"][0] < searched["far"][1]


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """tests/separation_emu.cpp with its own main and the library's host translation unit, built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run once: every lane of six seeded pairs, pruned and not, and the host entry over them."""
    exe = str(tmp_path / "separation_emu_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DSEPARATION_EMU_MAIN", "-o", exe, os.path.join(ROOT, "tests", "separation_emu.cpp"),
                           os.path.join(CSRC, "mtg_separation_host.cpp")], stderr=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "0 mismatches" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
