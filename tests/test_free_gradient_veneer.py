"""The gradient with respect to the free derivatives of the C++ compat veneer
(include/compat/mav_trajectory_generation/polynomial_optimization_linear.h): PolynomialOptimizationBatch<N>::freeGradientHost
over mtg_free_gradient_host (no device) on cases written out by hand, and PolynomialOptimizationBatch<N>::freeGradient over
mtg_free_gradient on the device, bit for bit against the host form."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_free_gradient_veneer")


def build_exe():
    src = os.path.join(ROOT, "tests", "cpp", "test_free_gradient_veneer.cpp")
    deps = [src, os.path.join(ROOT, "include", "mtg_hip.h"), os.path.join(ROOT, "include", "compat", "mtg_mini_eigen", "Eigen", "Core")]
    d = os.path.join(ROOT, "include", "compat", "mav_trajectory_generation")
    deps += [os.path.join(d, f) for f in os.listdir(d)]
    if os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(p) for p in deps):
        return
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include", "compat"), "-I" + os.path.join(ROOT, "include"),
                           "-o", EXE, src, "-L" + os.path.join(ROOT, "mav_trajectory_generation_amd", "csrc"), "-lmtg_hip", "-pthread",
                           "-Wl,-rpath,$ORIGIN/../../mav_trajectory_generation_amd/csrc"])


def test_free_gradient_veneer_on_the_host():
    build_exe()
    undefined = subprocess.run(["nm", "-D", "--undefined-only", EXE], capture_output=True, text=True).stdout
    assert "mtg_free_gradient_host" in undefined
    assert any(line.split()[-1] == "mtg_free_gradient" for line in undefined.splitlines() if line.split())
    r = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "FREE-GRADIENT VENEER TESTS PASSED (host)" in r.stdout


@pytest.mark.gpu
def test_free_gradient_veneer_on_the_device():
    build_exe()
    r = subprocess.run([EXE, "device"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "FREE-GRADIENT VENEER TESTS PASSED (host + device)" in r.stdout
