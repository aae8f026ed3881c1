"""Device time of the batched trajectory-to-trajectory separation check on the benchmark's own batch against itself: B solved
trajectories (10k x 8 segments, N = 10, D = 3) as B / 16 swarms of 16 with all 120 pairs each (75 000 pairs, 600 000 lanes).

Recorded, not gated -- no earlier call returns the same numbers, so there is no other side to beat:
  * `aligned`: one call, both sides the same buffers, no start times (every trajectory starts at 0);
  * `staggered`: the same call with a start time per trajectory on side B, so that no breakpoint of B coincides with one of A;
  * `spheres`: check_obstacle_clearance of the same batch against 8 spheres scattered in the waypoint box, for scale;
  * from the host build of the lane (tests/separation_emu.cpp, its search counter) on the first `--model` pairs: pieces and root
    searches per lane and per wave of 64 consecutive lanes, for both calls.

Protocol of tools/bench_obstacle_clearance.py: one process; device events around `--calls` back-to-back calls after a warm-up; the
inputs rotate over enough coefficient buffers that they come from HBM (more than 512 MB of them); the three calls alternate and
the round is repeated `--repeats` times; the median and the spread (max - min over the median) of each are reported.
Prints one JSON line; --out appends it to a file.

    python tools/bench_trajectory_separation.py [--batch 10000] [--calls 20] [--repeats 5] [--out profiles/trajectory_separation_bench.jsonl]
"""
import argparse
import ctypes
import json
import os
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


def lane_counter():
    """tests/separation_emu.cpp as a library: the lane with its search counter."""
    so, src = os.path.join(ROOT, "tests", "libmtg_separation_emu.so"), os.path.join(ROOT, "tests", "separation_emu.cpp")
    csrc = os.path.join(ROOT, "mav_trajectory_generation_amd", "csrc")
    deps = [src] + [os.path.join(csrc, h) for h in ("mtg_separation_lane.h", "mtg_obstacle_lane.h", "mtg_segment_lane.h", "mtg_extrema_lane.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    p = ctypes.c_void_p
    lib.separation_emu_lane.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, p, p, ctypes.c_double, ctypes.c_int, p, p, ctypes.c_double,
                                        ctypes.c_int, ctypes.c_double, ctypes.c_int, p, p]
    return lib


def lane_model(coeffs, times, start_b, pairs, min_separation):
    """Pieces and searches of every lane of `pairs` (in lane order), from the host build of the lane."""
    lib = lane_counter()
    k, d, n = coeffs.shape[1:]
    f, c = np.zeros(2), np.zeros(6, dtype=np.int32)
    pieces, searches = [], []
    for a, b in pairs:
        for i in range(k):
            assert lib.separation_emu_lane(n, d, k, coeffs[a].ctypes.data, times[a].ctypes.data, 0.0, k, coeffs[b].ctypes.data, times[b].ctypes.data,
                                           float(start_b[b]), i, min_separation, 1, f.ctypes.data, c.ctypes.data) == 0
            pieces.append(int(c[3]))
            searches.append(int(c[5]))
    pieces, searches = np.array(pieces), np.array(searches)
    waves = lambda x: x[: x.size // 64 * 64].reshape(-1, 64).max(axis=1)
    return {"pairs": len(pairs), "pieces_per_lane_mean": round(float(pieces.mean()), 2), "pieces_per_lane_max": int(pieces.max()),
            "searches_per_lane_mean": round(float(searches.mean()), 2), "searches_per_lane_max": int(searches.max()),
            "searches_per_wave_mean": round(float(waves(searches).mean()), 2), "searches_per_wave_max": int(waves(searches).max())}


def stats(runs):
    med = sorted(runs)[len(runs) // 2]
    return {"us": round(med, 1), "spread_percent": round(100.0 * (max(runs) - min(runs)) / med, 2), "runs_us": [round(x, 1) for x in runs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=10_000)
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--swarm", type=int, default=16)
    ap.add_argument("--min-separation", type=float, default=1.0)
    ap.add_argument("--spheres", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--model", type=int, default=240, help="pairs of the host-side pieces / searches count (0: none)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, K, D, B = 10, args.segments, 3, args.batch
    box = 10.0                                                  # random_waypoint_batch's
    swarms = B // args.swarm
    local = m.all_pairs(args.swarm)
    pairs = (local[None, :, :] + (np.arange(swarms, dtype=np.int32) * args.swarm)[:, None, None]).reshape(-1, 2)
    rng = np.random.default_rng(2024)
    stagger = rng.uniform(0.0, 2.0, B)                          # (a random start: no sum of segment times of A meets one of B)
    spheres = m.sphere_obstacles(rng.uniform(-box, box, (args.spheres, 3)), rng.uniform(0.5, 1.5, args.spheres))
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
        d_pairs, d_stagger, d_spheres = torch.from_numpy(pairs).cuda(), torch.from_numpy(stagger).cuda(), torch.from_numpy(spheres).cuda()

        def aligned(i):
            co, t = bufs[i % n_buf]
            return m.check_trajectory_separation(ctx, co, t, co, t, d_pairs, args.min_separation)

        def staggered(i):
            co, t = bufs[i % n_buf]
            return m.check_trajectory_separation(ctx, co, t, co, t, d_pairs, args.min_separation, start_b=d_stagger)

        def sphere_check(i):
            return m.check_obstacle_clearance(ctx, *bufs[i % n_buf], d_spheres)

        first = {"aligned": aligned(0), "staggered": staggered(0)}
        ctx.sync()
        verdicts = {k: {"feasible_pairs": int(v.pair_feasible.sum()), "pairs": int(v.pair_feasible.numel()),
                        "pieces_per_lane_mean": round(float(v.segment_pieces.double().mean()), 3),
                        "smallest_separation": float(v.pair_separation.min())} for k, v in first.items()}
        sides = {"aligned": aligned, "staggered": staggered, "spheres": sphere_check}
        for fn in sides.values():
            timed(ctx, fn, args.warmup)
        runs = {k: [] for k in sides}
        for _ in range(args.repeats):
            for name, fn in sides.items():
                runs[name].append(timed(ctx, fn, args.calls))
        model = None
        if args.model:
            co, t = bufs[0][0].cpu().numpy(), bufs[0][1].cpu().numpy()
            head = pairs[: args.model]
            model = {"aligned": lane_model(co, t, np.zeros(B), head, args.min_separation),
                     "staggered": lane_model(co, t, stagger, head, args.min_separation)}
        plan.close()
    out = {"tool": "bench_trajectory_separation", "N": N, "K": K, "D": D, "batch": B, "swarm": args.swarm, "pairs": int(len(pairs)),
           "lanes": int(len(pairs)) * K, "min_separation": args.min_separation, "calls": args.calls, "repeats": args.repeats, "buffers": n_buf,
           "aligned": dict(stats(runs["aligned"]), **verdicts["aligned"]), "staggered": dict(stats(runs["staggered"]), **verdicts["staggered"]),
           "spheres": dict(stats(runs["spheres"]), n=args.spheres), "model": model}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
