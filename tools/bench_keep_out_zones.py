"""Device time of the batched keep-out zone check (A), recorded, not gated: no earlier call gives the same numbers.

Protocol of tools/bench_obstacle_clearance.py: one process; device events around `--calls` back-to-back calls after a warm-up; the
inputs rotate over enough coefficient buffers that they come from HBM (more than 512 MB of them); the sides alternate and the
round is repeated `--repeats` times, the spread over the repeats is reported with the median.  Sides: A -- `--zones` axis-aligned
boxes scattered in the waypoint box (sizes 1 .. 3); A_unpruned -- the same centres with size 80: every segment lies INSIDE every
box, no bound is positive, nothing can be pruned, every lane runs all the searches of every zone; for scale, the sphere check on as
many spheres at the same centres (radii 0.5 .. 1.5), measured in the same run.  Next to the times: the zones searched per lane and
per wave of the scattered set from the lane code's own counter (tools/cpp/keep_out_searches.cpp, the host build of the lane header,
on the first `--model` trajectories), and -- with --remarks <dir of a MTG_BUILD_REMARKS build> -- VGPRs, AGPRs, scratch and LDS of
every instantiation.  Two conditions are asserted: the call on all zones returns bit for bit what the unpruned one-zone calls
combine to, and no instantiation uses scratch.  Prints one JSON line; --out appends it to a file.

    python tools/bench_keep_out_zones.py [--batch 10000] [--calls 100] [--repeats 5] [--remarks DIR] [--out profiles/keep_out_zones_bench.jsonl]
"""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import mav_trajectory_generation_amd as m  # noqa: E402


def timed(ctx, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(ctx.stream)
    for i in range(calls):
        fn(i)
    e1.record(ctx.stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def searches_per_lane(coeffs, times, zones):
    """[B K] zones searched per lane, from the lane code's counter."""
    src = os.path.join(ROOT, "tools", "cpp", "keep_out_searches.cpp")
    lib = os.path.join(ROOT, "tools", "cpp", "libkeep_out_searches.so")
    deps = [src] + [os.path.join(ROOT, "mav_trajectory_generation_amd", "csrc", h) for h in
                    ("mtg_keepout_lane.h", "mtg_obstacle_lane.h", "mtg_segment_lane.h", "mtg_extrema_lane.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call(["g++", "-O2", "-march=x86-64-v3", "-std=c++17", "-shared", "-fPIC", "-o", lib, src])
    so = ctypes.CDLL(lib)
    bsz, k, d, n = coeffs.shape
    coeffs, times, zones = (np.ascontiguousarray(a, dtype=np.float64) for a in (coeffs, times, zones))
    out = np.zeros((bsz, k), dtype=np.int32)
    so.keep_out_searches.argtypes = [ctypes.c_int32] * 3 + [ctypes.c_int64] + [ctypes.c_void_p] * 3 + [ctypes.c_int32] * 2 + [ctypes.c_double, ctypes.c_void_p]
    assert so.keep_out_searches(n, k, d, bsz, coeffs.ctypes.data, times.ctypes.data, zones.ctypes.data, zones.shape[0], zones.shape[1], 0.0,
                                out.ctypes.data) == 0
    return out.ravel()


def resources(remarks):
    """{instantiation: {vgprs, agprs, scratch, lds}} of the segment kernels, from the build's resource remarks."""
    text = open(os.path.join(remarks, "mtg_keepout.log")).read()
    out = {}
    for name, body in re.findall(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", text, flags=re.S):
        inst = re.search(r"seg_kernelILi(\d+)ELb([01])E", name)
        if not inst:
            continue
        get = lambda key: int(re.search(re.escape(key) + r": (\d+)", body).group(1))
        out[f"N{inst.group(1)}_{'shared' if inst.group(2) == '1' else 'per_trajectory'}"] = {
            "vgprs": get("VGPRs"), "agprs": get("AGPRs"), "scratch": get("ScratchSize [bytes/lane]"), "lds": get("LDS Size [bytes/block]")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=10_000)
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--zones", type=int, default=16)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--model", type=int, default=1024, help="trajectories the searches are counted on (0: none)")
    ap.add_argument("--remarks", default=None, help="directory of a MTG_BUILD_REMARKS build: resources per instantiation")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, K, D, B, M = 10, args.segments, 3, args.batch, args.zones
    box = 10.0                                                  # random_waypoint_batch's
    rng = np.random.default_rng(2024)
    centres = rng.uniform(-box, box, (M, 3))
    radii = rng.uniform(0.5, 1.5, M)
    scattered = m.keep_out_boxes(centres, rng.uniform(1.0, 3.0, (M, 3)))
    enclosing = m.keep_out_boxes(centres, [80.0, 80.0, 80.0])
    spheres = m.sphere_obstacles(centres, radii)
    res = resources(args.remarks) if args.remarks else None
    if res is not None:
        assert len(res) == 10 and all(r["scratch"] == 0 for r in res.values()), res
    ctx = m.Context(0)
    with torch.cuda.stream(ctx.stream):
        masks = m.ends_full_masks(N, K)
        plan = m.Plan(ctx, N, D, K, N // 2 - 1, masks)
        per_buffer = B * K * D * N * 8
        n_buf = max(2, (512 << 20) // per_buffer + 1)
        bufs = []
        for i in range(n_buf):
            t, f = m.random_waypoint_batch(B, K, D, N, masks, seed=8 + i, device="cuda", box=box)
            co, _, _ = plan.solve(t, f)
            bufs.append((co.clone(), t.clone()))
        ctx.sync()
        d_scattered, d_enclosing, d_spheres = (torch.from_numpy(a).cuda() for a in (scattered, enclosing, spheres))

        sides = {"a": lambda i: m.check_keep_out_zones(ctx, *bufs[i % n_buf], d_scattered),
                 "a_unpruned": lambda i: m.check_keep_out_zones(ctx, *bufs[i % n_buf], d_enclosing),
                 "spheres": lambda i: m.check_obstacle_clearance(ctx, *bufs[i % n_buf], d_spheres)}

        # the call on all zones against the unpruned one-zone calls, bit for bit
        identical = {}
        for name, zones in (("scattered", d_scattered), ("enclosing", d_enclosing)):
            full = m.check_keep_out_zones(ctx, *bufs[0], zones)
            singles = [m.check_keep_out_zones(ctx, *bufs[0], zones[h:h + 1].contiguous()) for h in range(M)]
            ctx.sync()
            host = lambda x: x.cpu().numpy()
            pair = np.stack([host(s.segment_clearance) for s in singles], axis=2)                    # [B][K][M]
            pair_t = np.stack([host(s.segment_closest_time) for s in singles], axis=2)
            assert not np.isnan(pair).any()
            nearest = pair.argmin(axis=2)                                                             # (the smallest index at the minimum)
            fails = ~(pair > 0.0)
            seg_fail = fails.any(axis=2)
            fseg = np.where(seg_fail.any(axis=1), seg_fail.argmax(axis=1), -1)
            fzone = np.array([-1 if k < 0 else int(fails[b, k].argmax()) for b, k in enumerate(fseg)])
            same = (np.array_equal(host(full.segment_clearance), pair.min(axis=2)) and np.array_equal(host(full.segment_nearest_zone), nearest)
                    and np.array_equal(host(full.segment_closest_time), np.take_along_axis(pair_t, nearest[:, :, None], axis=2)[:, :, 0])
                    and np.array_equal(host(full.first_failing_segment), fseg) and np.array_equal(host(full.first_failing_zone), fzone)
                    and np.array_equal(host(full.trajectory_feasible) != 0, ~seg_fail.any(axis=1))
                    and np.array_equal(host(full.trajectory_clearance), pair.min(axis=(1, 2))))
            assert same, name
            identical[name] = same
            if name == "scattered":
                feasible = int(full.trajectory_feasible.sum())
            else:
                assert not full.trajectory_feasible.any()      # every segment is inside every enclosing box

        for fn in sides.values():
            timed(ctx, fn, args.warmup)
        runs = {k: [] for k in sides}
        for _ in range(args.repeats):
            for name, fn in sides.items():
                runs[name].append(timed(ctx, fn, args.calls))
        model = None
        if args.model:
            nb = min(args.model, B)
            co, t = bufs[0][0][:nb].cpu().numpy(), bufs[0][1][:nb].cpu().numpy()
            per_lane = searches_per_lane(co, t, scattered)
            assert (searches_per_lane(co[:64], t[:64], enclosing) == M).all()
            per_wave = per_lane[: per_lane.size // 64 * 64].reshape(-1, 64).max(axis=1)
            model = {"trajectories": nb, "zones_per_lane_mean": round(float(per_lane.mean()), 2), "zones_per_lane_max": int(per_lane.max()),
                     "zones_per_wave_mean": round(float(per_wave.mean()), 2), "zones_per_wave_max": int(per_wave.max()), "of": M}
        plan.close()
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    spread = {k: round(100.0 * (max(v) - min(v)) / med[k], 2) for k, v in runs.items()}
    out = {"tool": "bench_keep_out_zones", "N": N, "K": K, "D": D, "batch": B, "zones": M, "planes": 6, "calls": args.calls,
           "repeats": args.repeats, "buffers": n_buf, "feasible_trajectories": feasible,
           "A_us": round(med["a"], 1), "A_unpruned_us": round(med["a_unpruned"], 1), "spheres_us": round(med["spheres"], 1),
           "spread_percent": spread, "A_runs_us": [round(x, 1) for x in runs["a"]],
           "A_unpruned_runs_us": [round(x, 1) for x in runs["a_unpruned"]], "spheres_runs_us": [round(x, 1) for x in runs["spheres"]],
           "identical_to_unpruned_one_zone_calls": identical, "searched": model, "resources": res}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
