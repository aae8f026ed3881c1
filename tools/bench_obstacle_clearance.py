"""Device time of the batched sphere-obstacle clearance check (A) against what the library offered before it for the same
numbers (B = per sphere an offset copy of the coefficients + minmax_magnitude(position, dimensions 0-2), then the tensor
reduction over the spheres).

Protocol of tools/bench_axis_minmax.py: one process; device events around `--calls` back-to-back calls after a warm-up; the inputs
rotate over enough coefficient buffers that they come from HBM (more than 512 MB of them); A and B alternate and the round is
repeated `--repeats` times: s = spread of B over the repeats, A < B counts as met at A < (1 - s / 100) B.  A is timed twice: 16
spheres scattered in the waypoint box (radii 0.5 .. 1.5), and the same centres with radius 40 -- every segment lies INSIDE every
sphere, no bound is positive, nothing can be pruned: all 16 searches in every lane.  Next to the times: the searches per lane and
per wave of the scattered set, from a host-side model on the first `--model` trajectories (the lane header's bound restated in
numpy, the clearances of every (segment, sphere) pair from one-sphere host calls, the walk in ascending (bound, index) order).
Prints one JSON line; --out appends it to a file.

    python tools/bench_obstacle_clearance.py [--batch 10000] [--calls 100] [--repeats 5] [--out profiles/obstacle_clearance_bench.jsonl]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import mav_trajectory_generation_amd as m  # noqa: E402

EPS = float(np.finfo(np.float64).eps)


def timed(ctx, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(ctx.stream)
    for i in range(calls):
        fn(i)
    e1.record(ctx.stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def split_half(ctrl):
    """de Casteljau at 1/2 along the last axis: the control polygons of the two halves."""
    pts = ctrl.copy()
    left, right = [pts[..., 0]], [pts[..., -1]]
    for _ in range(1, ctrl.shape[-1]):
        pts = 0.5 * (pts[..., :-1] + pts[..., 1:])
        left.append(pts[..., 0])
        right.append(pts[..., -1])
    return np.stack(left, axis=-1), np.stack(right[::-1], axis=-1)


def lower_bounds(coeffs, times, obstacles):
    """csrc/mtg_obstacle_lane.h: lower_bound() restated -- [B][K][M] from the Bernstein hulls of every segment's quarters (N even)."""
    n = coeffs.shape[-1]
    u = coeffs[:, :, :3, :] * times[:, :, None, None] ** np.arange(n)                     # [B][K][3][N]
    w = np.array([[math.comb(k, i) / math.comb(n - 1, i) if i <= k else 0.0 for i in range(n)] for k in range(n)])
    left, right = split_half(u @ w.T)                                                     # [B][K][3][N] control points, halved
    e = np.abs(u).sum(axis=-1)                                                            # [B][K][3]
    c, r = obstacles[:, :3], obstacles[:, 3]
    margin = 96.0 * EPS * (e[:, :, None, :] + np.abs(c))
    acc = np.inf
    for quarter in split_half(left) + split_half(right):
        lo, hi = quarter.min(axis=-1), quarter.max(axis=-1)
        gap = np.maximum(lo[:, :, None, :] - c, c - hi[:, :, None, :]) - margin
        acc = np.minimum(acc, (np.maximum(gap, 0.0) ** 2).sum(axis=-1))
    dist = np.sqrt(acc)
    return dist - r - 8.0 * EPS * (dist + r)


def searches_model(coeffs, times, obstacles):
    """Searches per lane ([B K]) of the walk in ascending (bound, index) order that stops at the first obstacle whose bound is > 0
    and above the running minimum."""
    pair = np.stack([m.check_obstacle_clearance_host(coeffs, times, obstacles[h:h + 1]).segment_clearance for h in range(len(obstacles))], axis=2)
    bound = lower_bounds(coeffs, times, obstacles)
    assert (bound <= pair).all()                                                           # a bound is a bound
    order = np.argsort(bound, axis=2, kind="stable")
    count = np.zeros(pair.shape[:2], dtype=np.int64)
    for b in range(pair.shape[0]):
        for k in range(pair.shape[1]):
            best = math.inf
            for h in order[b, k]:
                if bound[b, k, h] > 0.0 and bound[b, k, h] > best:
                    break
                best = min(best, pair[b, k, h])
                count[b, k] += 1
    return count.ravel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=10_000)
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--spheres", type=int, default=16)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--model", type=int, default=256, help="trajectories of the host-side searches-per-lane model (0: none)")
    ap.add_argument("--only", choices=["a", "a_unpruned", "b"], default=None, help="one side only, once (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, K, D, B, M = 10, args.segments, 3, args.batch, args.spheres
    box = 10.0                                                  # random_waypoint_batch's
    rng = np.random.default_rng(2024)
    centres = rng.uniform(-box, box, (M, 3))
    scattered = m.sphere_obstacles(centres, rng.uniform(0.5, 1.5, M))
    enclosing = m.sphere_obstacles(centres, 40.0)
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
        d_scattered, d_enclosing = torch.from_numpy(scattered).cuda(), torch.from_numpy(enclosing).cuda()
        spheres = [(torch.from_numpy(scattered[h, :3].copy()).cuda(), float(scattered[h, 3])) for h in range(M)]

        def a_side(i):
            return m.check_obstacle_clearance(ctx, *bufs[i % n_buf], d_scattered)

        def a_unpruned(i):
            return m.check_obstacle_clearance(ctx, *bufs[i % n_buf], d_enclosing)

        def b_side(i):
            co, t = bufs[i % n_buf]
            rows = []
            for centre, radius in spheres:
                shifted = co.clone()
                shifted[:, :, :, 0] -= centre
                rows.append(m.minmax_magnitude(ctx, shifted, t, 0, dimensions=[0, 1, 2])[0][:, :, 1] - radius)
            seg, nearest = torch.stack(rows, dim=2).min(dim=2)
            return seg, nearest, (seg > 0.0).all(dim=1), seg.min(dim=1).values

        a, b = a_side(0), b_side(0)
        ctx.sync()
        worst = float(((a.segment_clearance - b[0]).abs()).max())        # the two sides answer the same question
        assert worst <= 1e-6 * (3.0 * box + 2.0), worst        # (the loose side of the fixture rule; the figure is reported)
        assert torch.equal(a.trajectory_feasible != 0, b[2])
        feasible = int(a.trajectory_feasible.sum())

        sides = {"a": a_side, "a_unpruned": a_unpruned, "b": b_side}
        if args.only:
            us = timed(ctx, sides[args.only], args.calls)
            print(json.dumps({"only": args.only, "us": round(us, 1), "calls": args.calls}))
            return
        for fn in sides.values():
            timed(ctx, fn, args.warmup)
        runs = {k: [] for k in sides}
        for _ in range(args.repeats):
            for name, fn in sides.items():
                runs[name].append(timed(ctx, fn, args.calls))
        model = None
        if args.model:
            nb = min(args.model, B)
            per_lane = searches_model(bufs[0][0][:nb].cpu().numpy(), bufs[0][1][:nb].cpu().numpy(), scattered)
            per_wave = per_lane[: per_lane.size // 64 * 64].reshape(-1, 64).max(axis=1)
            model = {"trajectories": nb, "searches_per_lane_mean": round(float(per_lane.mean()), 2), "searches_per_lane_max": int(per_lane.max()),
                     "searches_per_wave_mean": round(float(per_wave.mean()), 2), "searches_per_wave_max": int(per_wave.max()), "of": M}
        plan.close()
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    spread = 100.0 * (max(runs["b"]) - min(runs["b"])) / med["b"]
    out = {"tool": "bench_obstacle_clearance", "N": N, "K": K, "D": D, "batch": B, "spheres": M, "calls": args.calls, "repeats": args.repeats,
           "buffers": n_buf, "feasible_trajectories": feasible,
           "A_us": round(med["a"], 1), "A_unpruned_us": round(med["a_unpruned"], 1), "B_us": round(med["b"], 1),
           "B_spread_percent": round(spread, 2), "A_runs_us": [round(x, 1) for x in runs["a"]],
           "A_unpruned_runs_us": [round(x, 1) for x in runs["a_unpruned"]], "B_runs_us": [round(x, 1) for x in runs["b"]],
           "A_vs_B_largest_difference": worst, "A_lt_B_met": bool(med["a"] < (1.0 - spread / 100.0) * med["b"]),
           "A_unpruned_lt_B_met": bool(med["a_unpruned"] < (1.0 - spread / 100.0) * med["b"]), "model": model}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
