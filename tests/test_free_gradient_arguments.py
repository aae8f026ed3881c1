"""Argument table of mtg_free_gradient_host and mtg_free_gradient.  Return codes only: what the accepted calls compute is the
matter of test_free_gradient.py.  The device entry checks its arguments before it uses its plan's context; without a device no
plan can exist, so here only its null-plan branch runs (refused, nothing read) and its argument rules are checked with a real
plan in tests/test_gpu_free_gradient.py.  The stand-alone sanitizer program is run from here too."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from mav_trajectory_generation_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mav_trajectory_generation_amd", "csrc")
OK, INVALID = 0, -1
B = 3

# (id, keyword arguments of call(), expected)
CASES = [
    ("plain", {}, OK),
    ("n_0", dict(N=0), INVALID), ("n_2", dict(N=2, d=0), OK), ("n_odd", dict(N=7), INVALID), ("n_12", dict(N=12), OK),
    ("n_14", dict(N=14), INVALID), ("k_0", dict(K=0), INVALID), ("k_1", dict(K=1), OK), ("dim_0", dict(D=0), INVALID),
    ("dim_1", dict(D=1), OK), ("dim_4", dict(D=4), OK), ("d_negative", dict(d=-1), INVALID), ("d_0", dict(d=0), OK),
    ("d_h_minus_1", dict(N=8, d=3), OK), ("d_h", dict(N=8, d=4), INVALID),
    ("batch_negative", dict(batch=-1), INVALID), ("batch_0", dict(batch=0), OK), ("batch_1", dict(batch=1), OK),
    ("null_desc", dict(null=("desc",)), INVALID), ("null_masks", dict(null=("masks",)), INVALID),
    ("null_layout", dict(null=("layout",)), INVALID), ("null_times", dict(null=("times",)), INVALID),
    ("grad_only", dict(null=("coeffs",)), OK), ("coeffs_only", dict(null=("grad",)), OK),
    ("no_input", dict(null=("grad", "coeffs")), INVALID),
    ("free_only", dict(null=("fixed",)), OK), ("fixed_only", dict(null=("free",)), OK),
    ("no_output", dict(null=("free", "fixed")), INVALID),
    ("weight_nan_without_coeffs", dict(w=float("nan"), null=("coeffs",)), OK), ("weight_inf", dict(w=float("inf")), OK),
    ("times_not_validated", dict(bad_times=True), OK),
    ("rank_deficient_plan", dict(masks="none"), OK), ("no_free_columns", dict(masks="full", null=("free",)), OK),
    ("high_mask_bits_ignored", dict(masks="high"), OK),
]


def call(N=10, K=3, D=3, d=2, batch=B, w=1.0, null=(), masks="standard", bad_times=False, device=False):
    lib = L.load()
    nn, nk, nd, nb = max(N, 2), max(K, 1), max(D, 1), max(batch, 1)
    h = nn // 2
    full = (1 << h) - 1
    mk = {"standard": [full] + [1] * (nk - 1) + [full], "none": [0] * (nk + 1), "full": [full] * (nk + 1),
          "high": [full | 0xffff0000] + [1 | (1 << h)] * (nk - 1) + [full]}[masks]
    rng = np.random.default_rng(7)
    times = rng.uniform(0.5, 2.0, (nb, nk))
    if bad_times:
        times[0, 0], times[-1, -1] = -1.0, float("nan")
    grad, coeffs = rng.standard_normal((nb, nk, nd, nn)), rng.standard_normal((nb, nk, nd, nn))
    free, fixed = np.empty((nb, nd, h * (nk + 1))), np.empty((nb, nd, h * (nk + 1)))
    arr = (ctypes.c_uint32 * (nk + 1))(*mk)
    desc = L.PlanDesc(N, D, K, d, None if "masks" in null else arr)
    lay = L.Layout(nk, 1, nd * h * (nk + 1), h * (nk + 1), 1, nd * h * (nk + 1), h * (nk + 1), 1)
    ptr = dict(times=times.ctypes.data, grad=grad.ctypes.data, coeffs=coeffs.ctypes.data, free=free.ctypes.data, fixed=fixed.ctypes.data,
               layout=ctypes.byref(lay), desc=ctypes.byref(desc))
    for name in null:
        if name != "masks":
            ptr[name] = None
    tail = [batch, ptr["layout"], ptr["times"], ptr["grad"], ptr["coeffs"], w, ptr["free"], ptr["fixed"]]
    if device:
        return lib.mtg_free_gradient(None, *tail)
    return lib.mtg_free_gradient_host(ptr["desc"], *tail)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_entry_rules(case):
    assert call(**case[1]) == case[2], case


def test_device_entry_refuses_a_null_plan_and_reads_nothing():
    """Only the null-plan branch of the device entry can run without a device: it must refuse and dereference nothing, whatever
    the other arguments are (null pointers included).  It says nothing about the entry's argument rules; those are checked with a
    real plan in tests/test_gpu_free_gradient.py::test_argument_table_with_a_real_plan."""
    for case in CASES:
        assert call(device=True, **case[1]) == INVALID, case


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "mtg_hip.h")).read()
    for name in ("mtg_free_gradient", "mtg_free_gradient_host"):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(L.EXPORTS[name][1]) == 9, name


def test_rule_is_stated_in_the_header_and_the_lane_header():
    for path in (os.path.join(ROOT, "include", "mtg_hip.h"), os.path.join(CSRC, "mtg_pullback_lane.h")):
        text = open(path).read()
        for phrase in ("tn_m = fl(tn_(m-1) ti)", "one fma(ai[j][k], u_j, z) per term from +0", "the left segment's end first"):
            assert phrase in text, (path, phrase)


def test_python_layer_refuses_a_call_without_inputs():
    import mav_trajectory_generation_amd as m
    with pytest.raises(m.MtgError):
        m.free_gradient_host(4, 1, [3, 3], np.ones((1, 1)))


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """tests/free_gradient_emu.cpp with its own main and the library's host translation unit, built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run once: every N, D in {1, 3, 4}, every combination of the optional pointers, guard words
    around both outputs, and a restatement of the rule that must agree bit for bit."""
    exe = str(tmp_path / "free_gradient_emu_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "free_gradient_emu.cpp"), os.path.join(CSRC, "mtg_pullback_host.cpp")],
                          stderr=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
