"""Argument table of mtg_collision_cost_host and mtg_collision_cost, after tests/test_trajectory_separation_arguments.py: the shape
rules the per-segment entries share, the distance-field check's own rows (the field, dt, max_samples, inflation), and this
entry's: a trilinear field only, epsilon > 0 and finite, speed_epsilon >= 0 and finite, segment_cost required, the other outputs
optional alone and together.  Return codes only: what the accepted calls compute is the matter of test_collision_cost.py.  The
device entry checks its arguments with the same predicate (csrc/mtg_collision_lane.h: arguments_ok) before it looks at its
context and returns for batch = 0 before it needs one: with a null context and an empty batch its table runs here, without a
device; with a batch, a null context is refused after the arguments.  The stand-alone sanitizer program is run from here too."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mav_trajectory_generation_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mav_trajectory_generation_amd", "csrc")
OK, INVALID = 0, -1
B, K = 3, 4
NAN, INF = float("nan"), float("inf")

# (id, N, K, D, batch, ts_b, ts_k, expected)
SHAPE_CASES = [
    ("n_0", 0, K, 3, B, K, 1, INVALID), ("n_1", 1, K, 3, B, K, 1, OK), ("n_odd", 7, K, 3, B, K, 1, OK), ("n_12", 12, K, 3, B, K, 1, OK),
    ("n_13", 13, K, 3, B, K, 1, INVALID), ("k_0", 10, 0, 3, B, 1, 1, INVALID), ("k_1", 10, 1, 3, B, 1, 1, OK),
    ("d_2", 10, K, 2, B, K, 1, INVALID), ("d_3", 10, K, 3, B, K, 1, OK), ("d_4", 10, K, 4, B, K, 1, OK), ("d_5", 10, K, 5, B, K, 1, INVALID),
    ("batch_minus_1", 10, K, 3, -1, K, 1, INVALID), ("batch_0", 10, K, 3, 0, K, 1, OK), ("batch_1", 10, K, 3, 1, K, 1, OK),
    ("ts_b_0", 10, K, 3, B, 0, 1, INVALID), ("ts_k_0", 10, K, 3, B, K, 0, INVALID), ("ts_k_negative", 10, K, 3, B, K, -1, INVALID),
    ("rows_bk_touching", 10, K, 3, B, K * 2, 2, OK), ("rows_bk_overlapping", 10, K, 3, B, K * 2 - 1, 2, INVALID),
    ("rows_kb_touching", 10, K, 3, B, 2, B * 2, OK), ("rows_kb_overlapping", 10, K, 3, B, 2, B * 2 - 1, INVALID),
    ("soa", 10, K, 3, B, 1, B, OK),
]

# (id, keyword arguments of call(), expected): the field check's own rows, then this entry's
RULE_CASES = [
    ("plain", {}, OK),
    ("nearest_field", dict(interpolation=0), INVALID), ("unknown_interpolation", dict(interpolation=2), INVALID),
    ("nx_1", dict(n=(1, 3, 3)), INVALID), ("ny_1", dict(n=(3, 1, 3)), INVALID), ("nz_1", dict(n=(3, 3, 1)), INVALID),
    ("n_2", dict(n=(2, 2, 2)), OK), ("nx_0", dict(n=(0, 3, 3)), INVALID),
    ("too_many_voxels", dict(n=(1 << 11, 1 << 11, 1 << 9), fake_grid=True), INVALID),
    ("voxel_size_0", dict(voxel_size=0.0), INVALID), ("voxel_size_negative", dict(voxel_size=-0.25), INVALID),
    ("voxel_size_nan", dict(voxel_size=NAN), INVALID), ("voxel_size_inf", dict(voxel_size=INF), INVALID),
    ("voxel_size_denormal", dict(voxel_size=5e-324), INVALID),
    ("origin_nan", dict(origin=(0.0, NAN, 0.0)), INVALID), ("origin_inf", dict(origin=(0.0, 0.0, INF)), INVALID),
    ("outside_nan", dict(outside=NAN), INVALID), ("outside_inf", dict(outside=INF), OK), ("outside_minus_inf", dict(outside=-INF), OK),
    ("dt_0", dict(dt=0.0), INVALID), ("dt_negative", dict(dt=-0.1), INVALID), ("dt_nan", dict(dt=NAN), INVALID), ("dt_inf", dict(dt=INF), INVALID),
    ("max_samples_1", dict(max_samples=1), INVALID), ("max_samples_2", dict(max_samples=2), OK),
    ("max_samples_2_20", dict(max_samples=1 << 20), OK), ("max_samples_beyond", dict(max_samples=(1 << 20) + 1), INVALID),
    ("inflation_negative", dict(inflation=-1e-300), INVALID), ("inflation_nan", dict(inflation=NAN), INVALID),
    ("inflation_inf", dict(inflation=INF), INVALID),
    ("epsilon_0", dict(epsilon=0.0), INVALID), ("epsilon_negative", dict(epsilon=-0.5), INVALID), ("epsilon_nan", dict(epsilon=NAN), INVALID),
    ("epsilon_inf", dict(epsilon=INF), INVALID), ("epsilon_tiny", dict(epsilon=1e-300), OK),
    ("speed_epsilon_0", dict(speed_epsilon=0.0), OK), ("speed_epsilon_negative", dict(speed_epsilon=-1e-300), INVALID),
    ("speed_epsilon_nan", dict(speed_epsilon=NAN), INVALID), ("speed_epsilon_inf", dict(speed_epsilon=INF), INVALID),
    ("null_coeffs", dict(null=("coeffs",)), INVALID), ("null_times", dict(null=("times",)), INVALID),
    ("null_field", dict(null=("field",)), INVALID), ("null_distances", dict(null=("distances",)), INVALID),
    ("null_segment_cost", dict(null=("segment_cost",)), INVALID),
]

OPTIONAL = ("trajectory_cost", "coeff_gradient", "segment_samples")


def call(N=10, k=K, D=3, batch=B, ts_b=K, ts_k=1, n=(5, 4, 3), voxel_size=0.25, origin=(0.0, 0.0, 0.0), outside=0.0, interpolation=1,
         dt=0.25, max_samples=64, inflation=0.1, epsilon=0.5, speed_epsilon=1e-3, null=(), wanted=OPTIONAL, device=False, fake_grid=False):
    """The entry's return code; buffers sized for the accepted reading of the arguments."""
    lib = L.load()
    nb, nk, nd, nn = max(batch, 1), max(k, 1), max(D, 1), max(N, 1)
    if nb * nk > 1 << 20:      # (a refused size is never read)
        nb = nk = 1
    coeffs = np.random.default_rng(1000 * nn + nd).standard_normal((nb, nk, nd, nn)) * 0.3
    times = np.ones(((nb - 1) * max(ts_b, 0) + (nk - 1) * max(ts_k, 0) + 1,))
    grid = np.ones((2, 2, 2) if fake_grid else tuple(max(x, 1) for x in n[::-1]), dtype=np.float32)   # (a refused count is never read)
    field = L.DistanceFieldC(None if "distances" in null else grid.ctypes.data, n[0], n[1], n[2], (ctypes.c_double * 3)(*origin), voxel_size,
                             outside, interpolation)
    out = dict(segment_cost=np.empty(nb * nk), trajectory_cost=np.empty(nb), coeff_gradient=np.empty(nb * nk * nd * nn),
               segment_samples=np.empty(nb * nk, dtype=np.int32))
    ptr = {name: (a.ctypes.data if name == "segment_cost" or name in wanted else None) for name, a in out.items()}
    ptr.update(coeffs=coeffs.ctypes.data, times=times.ctypes.data, field=ctypes.byref(field))
    for name in null:
        ptr[name] = None
    args = [N, k, D, batch, ptr["coeffs"], ptr["times"], ts_b, ts_k, ptr["field"], dt, max_samples, inflation, epsilon, speed_epsilon,
            ptr["segment_cost"], ptr["trajectory_cost"], ptr["coeff_gradient"], ptr["segment_samples"]]
    if device:
        return lib.mtg_collision_cost(None, *args)
    return lib.mtg_collision_cost_host(*args)


@pytest.mark.parametrize("case", SHAPE_CASES, ids=[c[0] for c in SHAPE_CASES])
def test_shape_rules(case):
    name, N, k, D, batch, ts_b, ts_k, expected = case
    assert call(N, k, D, batch, ts_b, ts_k) == expected, case


@pytest.mark.parametrize("case", RULE_CASES, ids=[c[0] for c in RULE_CASES])
def test_field_and_potential_rules(case):
    assert call(**case[1]) == case[2], case


@pytest.mark.parametrize("mask", range(8))
def test_optional_outputs_alone_and_together(mask):
    assert call(wanted=tuple(o for i, o in enumerate(OPTIONAL) if mask >> i & 1)) == OK


@pytest.mark.parametrize("case", SHAPE_CASES, ids=[c[0] for c in SHAPE_CASES])
def test_device_entry_shape_rules_without_a_device(case):
    """With an empty batch (the rows that vary the batch keep theirs; the two overlap rows need a batch to overlap in)."""
    name, N, k, D, batch, ts_b, ts_k, expected = case
    if name.endswith("overlapping"):
        expected = OK
    if name == "batch_1":      # a batch to work on and no context: refused after the arguments
        expected = INVALID
    assert call(N, k, D, batch if name.startswith("batch") else 0, ts_b, ts_k, device=True) == expected, case


@pytest.mark.parametrize("case", RULE_CASES, ids=[c[0] for c in RULE_CASES])
def test_device_entry_field_and_potential_rules_without_a_device(case):
    assert call(batch=0, device=True, **case[1]) == case[2], case


def test_device_entry_needs_a_context_only_after_its_arguments():
    for mask in range(8):
        wanted = tuple(o for i, o in enumerate(OPTIONAL) if mask >> i & 1)
        assert call(batch=0, device=True, wanted=wanted) == OK
        assert call(device=True, wanted=wanted) == INVALID
    # batch x n_segments beyond one launch: refused before anything is read (the host form has no such limit to test cheaply)
    assert call(k=(1 << 19) - 1, batch=1 << 13, ts_b=(1 << 19) - 1, device=True, null=("trajectory_cost",), wanted=()) == INVALID


def test_header_and_binding_agree():
    import re
    text = open(os.path.join(ROOT, "include", "mtg_hip.h")).read()
    for name in ("mtg_collision_cost", "mtg_collision_cost_host"):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(L.EXPORTS[name][1]), name
    assert len(L.EXPORTS["mtg_collision_cost"][1]) == 19 and len(L.EXPORTS["mtg_collision_cost_host"][1]) == 18


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """tests/collision_cost_emu.cpp with its own main and the library's host translation units, built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run once: seeded batches of every N and D through the host entry, guard words around every
    output, every combination of the optional outputs, and a restatement of the rule that must agree bit for bit."""
    exe = str(tmp_path / "collision_cost_emu_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "collision_cost_emu.cpp"), os.path.join(CSRC, "mtg_collision_host.cpp"),
                           os.path.join(CSRC, "mtg_field_host.cpp")], stderr=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "0 mismatches" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
