"""FeasibilityRecursive of the C++ compat veneer (include/compat/mav_trajectory_generation_ros/feasibility_recursive.h): Settings,
the reference's three constructors, checkInputFeasibility(Segment) over mtg_check_input_feasibility_recursive_host (no device) and
the inherited checkInputFeasibilityTrajectory, against eight rows of the reference's verdicts."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_recursive_feasibility_veneer")
ROWS = os.path.join(ROOT, "tests", "golden", "reference_recursive_feasibility_veneer_rows.txt")


def build_exe():
    src = os.path.join(ROOT, "tests", "cpp", "test_recursive_feasibility_veneer.cpp")
    deps = [src, os.path.join(ROOT, "include", "mtg_hip.h"), os.path.join(ROOT, "include", "compat", "mtg_mini_eigen", "Eigen", "Core")]
    for sub in ("mav_trajectory_generation", "mav_trajectory_generation_ros"):
        d = os.path.join(ROOT, "include", "compat", sub)
        deps += [os.path.join(d, f) for f in os.listdir(d)]
    if os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(p) for p in deps):
        return
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include", "compat"), "-I" + os.path.join(ROOT, "include"),
                           "-o", EXE, src, "-L" + os.path.join(ROOT, "mav_trajectory_generation_amd", "csrc"), "-lmtg_hip", "-pthread",
                           "-Wl,-rpath,$ORIGIN/../../mav_trajectory_generation_amd/csrc"])


def test_recursive_feasibility_veneer_on_the_host():
    build_exe()
    undefined = subprocess.run(["nm", "-D", "--undefined-only", EXE], capture_output=True, text=True).stdout
    assert "mtg_check_input_feasibility_recursive_host" in undefined
    r = subprocess.run([EXE, ROWS], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "RECURSIVE FEASIBILITY VENEER TESTS PASSED (host)" in r.stdout
