"""The certified distance-field check of the C++ compat veneer (include/compat/mav_trajectory_generation/trajectory_batch.h):
mtgCertifyDistanceField over mtg_certify_distance_field_host (one Trajectory; no device) and TrajectoryBatch::certifyDistanceField
over mtg_certify_distance_field, on straight lines through fields linear in one axis, with answers known by hand."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_certified_field_veneer")


def build_exe():
    src = os.path.join(ROOT, "tests", "cpp", "test_certified_field_veneer.cpp")
    deps = [src, os.path.join(ROOT, "include", "mtg_hip.h"), os.path.join(ROOT, "include", "compat", "mtg_mini_eigen", "Eigen", "Core")]
    d = os.path.join(ROOT, "include", "compat", "mav_trajectory_generation")
    deps += [os.path.join(d, f) for f in os.listdir(d)]
    if os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(p) for p in deps):
        return
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include", "compat"), "-I" + os.path.join(ROOT, "include"),
                           "-o", EXE, src, "-L" + os.path.join(ROOT, "mav_trajectory_generation_amd", "csrc"), "-lmtg_hip", "-pthread",
                           "-Wl,-rpath,$ORIGIN/../../mav_trajectory_generation_amd/csrc"])


def test_certified_field_veneer_on_the_host():
    build_exe()
    undefined = subprocess.run(["nm", "-D", "--undefined-only", EXE], capture_output=True, text=True).stdout
    names = [line.split()[-1] for line in undefined.splitlines() if line.split()]
    assert "mtg_certify_distance_field_host" in names and "mtg_certify_distance_field" in names and "mtg_distance_field_lipschitz_host" in names
    r = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "CERTIFIED-FIELD VENEER TESTS PASSED (host)" in r.stdout


@pytest.mark.gpu
def test_certified_field_veneer_on_the_device():
    build_exe()
    r = subprocess.run([EXE, "device"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "CERTIFIED-FIELD VENEER TESTS PASSED (host + device)" in r.stdout
