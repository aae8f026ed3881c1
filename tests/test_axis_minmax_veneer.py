"""TrajectoryBatch::computeAxisMinMax and boundingBoxes of the C++ compat veneer (include/compat/mav_trajectory_generation/
trajectory_batch.h) over mtg_minmax_axes, against the veneer's own single-object Polynomial::computeMinMax."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_axis_minmax_veneer")


def build_exe():
    src = os.path.join(ROOT, "tests", "cpp", "test_axis_minmax_veneer.cpp")
    deps = [src, os.path.join(ROOT, "include", "mtg_hip.h"), os.path.join(ROOT, "include", "compat", "mtg_mini_eigen", "Eigen", "Core")]
    d = os.path.join(ROOT, "include", "compat", "mav_trajectory_generation")
    deps += [os.path.join(d, f) for f in os.listdir(d)]
    if os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(p) for p in deps):
        return
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include", "compat"), "-I" + os.path.join(ROOT, "include"),
                           "-o", EXE, src, "-L" + os.path.join(ROOT, "mav_trajectory_generation_amd", "csrc"), "-lmtg_hip", "-pthread",
                           "-Wl,-rpath,$ORIGIN/../../mav_trajectory_generation_amd/csrc"])


def test_axis_minmax_veneer_builds_on_the_device_entry():
    build_exe()
    undefined = subprocess.run(["nm", "-D", "--undefined-only", EXE], capture_output=True, text=True).stdout
    assert "mtg_minmax_axes" in undefined and "mtg_minmax_axes_host" not in undefined


@pytest.mark.gpu
def test_axis_minmax_veneer_on_the_device():
    build_exe()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "AXIS MINMAX VENEER TESTS PASSED (device)" in r.stdout
