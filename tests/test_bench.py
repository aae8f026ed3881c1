"""bench.py contract tests.  CPU: `--gpus 2` spawns two ranks by itself (no external launcher), rendezvous over gloo on
127.0.0.1, reports n_gpus == 2; a launcher / --gpus mismatch fails loudly.  GPU (1-GPU box): the full two-rank bench with
both ranks on device 0 over gloo, including the chunked solve + all_gather measurement."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*argv, env=None, timeout=600):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    if env:
        e.update(env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(argv), capture_output=True, text=True,
                          cwd=ROOT, env=e, timeout=timeout)


def last_json(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert lines, stdout
    return json.loads(lines[-1])


def test_gpus_flag_spawns_the_ranks_itself():
    r = run_bench("--gpus", "2", "--backend", "gloo", "--plumbing-only", "--steps", "3", "--warmup", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    out = last_json(r.stdout)
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1
    assert out["ranks_seen"] == 2 and out["rank_devices"] == [0, 1]     # an all_reduce of ones / all_gather of LOCAL_RANK


def test_world_size_mismatch_fails_loudly():
    r = run_bench("--gpus", "4", "--plumbing-only", env={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=2" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_two_rank_bench_on_one_gpu():
    r = run_bench("--gpus", "2", "--backend", "gloo", "--same-device", "--steps", "10", "--warmup", "3", "--batch", "4000",
                  "--buffer-sets", "2", "--no-cpu-baseline", "--gather-chunks", "2", "--full")
    assert r.returncode == 0, r.stderr[-3000:]
    out = last_json(r.stdout)
    assert out["n_gpus"] == 2 and out["steps"] == 10 and out["scaling"] == "weak"
    assert out["value"] > 0 and out["roofline"]["frac"] > 0
    g = out["gather"]
    assert g["chunks"] == 2 and g["solve_plus_gather_ms"] > 0 and g["gathered_bytes_per_rank"] == 2 * 4000 * 8 * 3 * 10 * 8
    # what a SCALE record needs beyond the contract fields: proof that the backend spans the ranks, where each rank ran,
    # every rank's own timing (value uses the max), and the CPU baseline when asked for
    assert out["ranks_seen"] == 2 and out["rank_devices"] == [0, 0]
    assert [r["rank"] for r in out["per_rank"]] == [0, 1] and all(r["device_us_per_step"] > 0 for r in out["per_rank"])
    assert out["roofline"]["device_us_per_step"] == max(r["device_us_per_step"] for r in out["per_rank"])
    assert all(0 < r["roofline_frac"] < 1 and r["units_per_s"] > 0 for r in out["per_rank"])
    assert abs(out["roofline"]["frac"] - min(r["roofline_frac"] for r in out["per_rank"])) < 1e-9
    assert out["parity"]["ok"] and out["parity"]["n"] >= 512       # rank 0's timed launch, checked against the oracles


@pytest.mark.gpu
@pytest.mark.parametrize("launcher", [False, True])
def test_rccl_branches_run_on_a_one_rank_group(launcher):
    """The `nccl` (= RCCL) branches of the N > 1 path -- init with a device id, all_reduce / all_gather of device tensors,
    barrier, the chunked solve overlapped with all_gather_into_tensor on the communication stream -- executed on the GPU
    box's one device (a one-rank group): everything but the cross-device transport itself.  launcher=True: under the very
    command the driver uses for N > 1 (python -m torch.distributed.run ... bench.py --gpus N), with N = 1."""
    argv = ["--gpus", "1", "--exercise-collectives", "--steps", "6", "--warmup", "2", "--batch", "4000", "--buffer-sets", "2",
            "--no-cpu-baseline", "--no-extras", "--gather-chunks", "2", "--full"]
    if launcher:
        e = dict(os.environ)
        for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
            e.pop(k, None)
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                            "--master-addr", "127.0.0.1", "--master-port", "29731", os.path.join(ROOT, "bench.py")] + argv,
                           capture_output=True, text=True, cwd=ROOT, env=e, timeout=600)
    else:
        r = run_bench(*argv)
    assert r.returncode == 0, r.stderr[-3000:]
    out = last_json(r.stdout)
    ce = out["collectives_exercised"]
    assert ce["backend"] == "nccl" and ce["ranks_seen"] == 1 and any("all_gather_into_tensor" in c for c in ce["calls"])
    assert out["n_gpus"] == 1 and out["gather"]["backend"] == "nccl" and out["gather"]["solve_plus_gather_ms"] > 0
    assert out["gather"]["own_slice_matches_local_solve"] is True
    # ... and the same chunked solve + gather through the C ABI's own RCCL communicator (mtg_comm_*), bit-identical to it
    via = out["gather"]["via_mtg_comm"]
    assert "error" not in via, via
    assert via["own_slice_matches_local_solve"] is True and via["matches_torch_distributed_gather"] is True and via["solve_plus_gather_ms"] > 0
    assert out["per_rank"][0]["device_us_per_step"] > 0 and out["parity"]["ok"]


@pytest.mark.gpu
def test_watchdog_falls_back_when_the_second_communicator_cannot_be_set_up():
    """The north-star gather (mtg_comm_*) is measured by default at every N; its ncclCommInitRank and first collectives run on a
    watchdog thread.  A rank that never comes back from them (simulated: MTG_BENCH_TEST_COMM_HANG) must not hang the run: the line
    is printed with the torch.distributed figures, says that it fell back, and the process exits 0 through os._exit."""
    import time
    t0 = time.time()
    r = run_bench("--gpus", "1", "--exercise-collectives", "--steps", "6", "--warmup", "2", "--batch", "4000", "--buffer-sets", "2",
                  "--no-cpu-baseline", "--no-extras", "--gather-chunks", "2", "--mtg-comm-init-timeout", "3", "--full",
                  env={"MTG_BENCH_TEST_COMM_HANG": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    assert time.time() - t0 < 300
    out = last_json(r.stdout)
    via = out["gather"]["via_mtg_comm"]
    assert "did not complete" in via["error"] and "torch.distributed" in via["fell_back"]
    assert out["gather"]["solve_plus_gather_ms"] > 0 and out["gather"]["own_slice_matches_local_solve"] is True


@pytest.mark.gpu
def test_two_rank_bench_carries_the_cpu_baseline():
    r = run_bench("--gpus", "2", "--backend", "gloo", "--same-device", "--steps", "4", "--warmup", "2", "--batch", "2000",
                  "--buffer-sets", "2", "--no-gather", "--no-extras", "--full")
    assert r.returncode == 0, r.stderr[-3000:]
    out = last_json(r.stdout)
    assert out["n_gpus"] == 2 and out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["cores"] >= 1


@pytest.mark.gpu
def test_single_gpu_bench_line_has_the_contract_fields():
    r = run_bench("--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--full")
    assert r.returncode == 0, r.stderr[-3000:]
    out = last_json(r.stdout)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in out
    assert out["n_gpus"] == 1 and out["dtype"] == "f64" and out["config"]["buffer_sets"] >= 25   # (>= steps + warmup sets and >= 1.25 GiB: the timed steps touch no set the warm-up used)
    rf = out["roofline"]
    assert rf["bound"] == "hbm" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    # HBM bytes per launch: measured by the invocation itself (round 6: child runs of the same command under rocprofv3 --pmc), or --
    # where rocprofv3 is not to be had -- from the committed PMC profile of this very command (null only when none is committed)
    if rf["traffic"] is not None:
        tp = rf["traffic_from_profile"]
        if tp.get("file") is None:
            assert "this invocation" in tp["measured"] and tp["kernel"].startswith("void mtg_solve_slab_queue_kernel")
        else:
            assert tp["bench_args_of_the_profile"].split()[:4] == ["--steps", "20", "--warmup", "5"]
        assert abs(rf["traffic"] - tp["hbm_bytes_per_step"] * 20) < 1.0
        assert 0.95 < rf["traffic_over_algorithmic"] < 1.2
    # round 6: the sustained figure is a first-class field (>= 1 s of continuous queue launches, shader clock probed next to them)
    su = out["sustained"]
    assert su["seconds"] > 0.5 and su["steps"] >= 1000 and 0.2 < su["roofline_frac"] < 1.0 and 500 < su["shader_clock_mhz"] < 3000
    assert out["value_aos_inputs"]["input_layout"] == "aos" and out["value_aos_inputs"]["value"] > 0
    # the 20 timed steps = 20 independent batches in ONE persistent launch (mtg_solve_linear_sequence)
    assert out["config"]["sequence"] == "queue" and rf["launches"] == 1 and rf["batches_per_launch"] == 20
    assert rf["bytes_per_launch"] == 20 * 10_000 * 2392 and rf["bytes_per_step"] == 10_000 * 2392
    assert abs(rf["achieved"] - rf["bytes_per_step"] / rf["device_us_per_step"] * 1e-3) < 1e-6 * rf["achieved"]
    assert out["ranks_seen"] == 1
    # the wall clock of the timed region is broken down, and the region a fresh process measures FIRST (idle GPU) is kept
    # beside the one after the settle phase
    w = out["timed_region_wall_us"]
    assert abs(w["enqueue_call"] + w["until_stop_event"] + w["barrier_and_synchronize"] - w["wall"]) < 1e-6 * w["wall"]
    assert out["settle_ms"] == 50.0 and out["cold_start"]["kernel_us_per_step"] > 0 and 0 < out["cold_start"]["frac"] < 1
    assert 0 < out["value_cold"] and abs(out["value_cold"] - out["cold_start"]["units_per_s_this_rank"]) < 1e-6 * out["value_cold"]
    # the metric's second half: coefficient rel-err of the TIMED launch's outputs vs the oracles, >= 512 trajectories over
    # >= 3 buffer sets, every sampled row NaN-prefilled and rewritten by the timed launch
    par = out["parity"]
    assert par["n"] >= 512 and len(set(par["buffer_sets_sampled"])) >= 3 and par["rows_not_written_by_the_timed_launch"] == 0
    assert par["tol"] == 1e-9 and par["ok"] and par["max_rel_err_vs_port"] <= 1e-9, par
    assert par["max_rel_err_vs_reference_build"] is None or par["max_rel_err_vs_reference_build"] <= 1e-9
    # the per-step hand-over form under the same protocol, as a peer of `value`
    peer = out["value_other_form"]
    assert peer["sequence"] == "launches" and peer["steps"] == 20 and 0 < peer["value"] < out["value"] * 1.05
    assert "cold_start" in out["config"]["workload"]
    assert "resident_buffers" in out["extra"]
    one = out["extra"]["one_launch_per_batch"]          # the latency form: reported beside, never as `value`
    assert one["steps"] == 200 and one["us_per_step"] > rf["device_us_per_step"]
    nx = out["extra"]["next"]                           # SURVEY 8(f) rows in the default line
    assert nx["sample"]["roofline"]["frac"] > 0 and nx["extrema"]["us"] > 0 and nx["mellinger"]["us"] > 0 and nx["time_scaling"]["us"] > 0


@pytest.mark.gpu
def test_latency_form_and_config4_lines():
    r = run_bench("--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--sequence", "launches", "--no-extras")
    assert r.returncode == 0, r.stderr[-3000:]
    out = last_json(r.stdout)
    assert out["config"]["sequence"] == "launches" and out["roofline"]["launches"] == 20
    assert out["roofline"]["bytes_per_launch"] == 10_000 * 2392
    r = run_bench("--config", "4", "--steps", "10", "--warmup", "3", "--buffer-sets", "4", "--full")
    assert r.returncode == 0, r.stderr[-3000:]
    out = last_json(r.stdout)
    # 12 buckets x 2500: sum over buckets of 8 * (K + 3 (N + K - 1) + 3 K N) bytes per trajectory = 128.9 MB per step
    want = sum(2500 * 8 * (k + 3 * (n + k - 1) + k * 3 * n) for n in (8, 10, 12) for k in (4, 8, 16, 32))
    assert out["config"]["baseline_config"] == 4 and out["config"]["trajectories_per_step"] == 30_000
    assert out["roofline"]["bytes_per_step"] == want and 0 < out["roofline"]["frac"] < 1
    assert out["roofline"]["launches"] == 1 and out["roofline"]["batches_per_launch"] == 10     # 10 requests, one launch
    assert out["extra"]["one_launch_per_request"]["us_per_step"] > 0
    assert "cpu_baseline" not in out
    # parity of the timed launch per polynomial order; the request is pre-built outside the timed region and says so
    par = out["parity"]
    assert par["ok"] and set(par["per_n"]) == {"8", "10", "12"} and all(v["n"] >= 512 for v in par["per_n"].values()), par
    # N <= 10 within 1e-9 of both oracles -- or, for the rare long ill-conditioned N = 10 chain on which the float64 oracles are
    # themselves ~1e-8 off, within 1e-9 of the 50-digit solution (the bench arbitrates every sample above the tolerance)
    assert par["per_n"]["8"]["max_rel_err_vs_port"] <= 1e-9 and par["per_n"]["10"]["ok"]
    if par["per_n"]["10"]["max_rel_err_vs_port"] > 1e-9:
        arb = par["above_tol_arbitrated_by_the_50_digit_solution"]
        assert arb and all(a["gpu_vs_50_digit_solution"] <= 1e-9 for a in arb), arb
    # round 5: the 240-item request is built INSIDE the timed region (`value` pays for it) and costs a fraction of it
    rb = out["request_build"]
    assert rb["inside_timed_region"] and 0 < rb["mtg_multi_create_us"] <= rb["host_us"]
    assert rb["share_of_timed_region_wall"] <= 0.25, rb
    assert out["value_other_form"]["sequence"] == "launches" and out["value_other_form"]["value"] > 0


def test_plain_and_full_options_are_there():
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """A plain run (no --full) measures only the headline figure; --dump-outputs writes the coefficients the LAST timed step
    wrote, the same from run to run, and they are what the library computes for that step's inputs."""
    import numpy as np
    outs = []
    for run in ("a", "b"):
        r = run_bench("--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path / run))
        assert r.returncode == 0, r.stderr[-3000:]
        out = last_json(r.stdout)
        assert out["steps"] == 7 and out["ms_per_step"] > 0 and out["value"] > 0 and out["dtype"] == "f64"
        assert abs(out["value"] - 10_000 / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
        for k in ("parity", "cpu_baseline", "extra", "gather"):
            assert k not in out, k
        assert out["cold_start"] is None and out["sustained"] is None and out["value_other_form"] is None
        assert sorted(os.listdir(tmp_path / run)) == ["coeffs.npy"]
        outs.append(np.load(tmp_path / run / "coeffs.npy"))
    assert outs[0].dtype == np.float64 and outs[0].shape == (10_000, 8, 3, 10) and np.isfinite(outs[0]).all()
    assert np.array_equal(outs[0], outs[1])
    # the last of the 2 + 7 steps used buffer set 8 of the rotation (>= 16 sets): seed 1234 + 1000 * 8, SoA inputs
    import torch
    import mav_trajectory_generation_amd as m
    masks = m.ends_full_masks(10, 8)
    ctx = m.Context(0)
    plan = m.Plan(ctx, 10, 3, 8, 4, masks)
    t, f = m.random_waypoint_batch(10_000, 8, 3, 10, masks, seed=1234 + 1000 * 8, device="cuda", layout="soa")
    co, _, _ = plan.solve(t, f, layout="soa")
    ctx.sync()
    want = co.cpu().numpy()
    plan.close()
    ctx.close()
    assert np.abs(outs[0] - want).max() <= 1e-9 * np.abs(want).max()
