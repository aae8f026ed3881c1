"""Device time of the batched per-axis extrema (A) against what the library offered before them for the per-axis |velocity| and
|acceleration| maxima (B = six minmax_magnitude calls: two derivatives x three one-bit dimension masks).

Protocol of tools/bench_half_plane.py: one process; device events around `--calls` back-to-back calls after a warm-up; the inputs
rotate over enough coefficient buffers that they come from HBM (more than 512 MB of them); A and B alternate and the round is
repeated `--repeats` times: s = spread of B over the repeats, A < B counts as met at A < (1 - s / 100) B.  A is timed twice:
velocity and acceleration (first = 1, n = 2, no trajectory outputs) and position .. snap (first = 0, n = 5).  Prints one JSON line;
--out appends it to a file.

    python tools/bench_axis_minmax.py [--batch 10000] [--calls 100] [--repeats 5] [--out profiles/axis_minmax_bench.jsonl]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=10_000)
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["a_va", "a_all", "b"], default=None, help="one side only, once (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, K, D, B = 10, args.segments, 3, args.batch
    ctx = m.Context(0)
    with torch.cuda.stream(ctx.stream):
        masks = m.ends_full_masks(N, K)
        plan = m.Plan(ctx, N, D, K, N // 2 - 1, masks)
        per_buffer = B * K * D * N * 8
        n_buf = max(2, (512 << 20) // per_buffer + 1)
        bufs = []
        for i in range(n_buf):
            t, f = m.random_waypoint_batch(B, K, D, N, masks, seed=8 + i, device="cuda")
            co, _, _ = plan.solve(t, f)
            bufs.append((co.clone(), t.clone()))
        ctx.sync()

        def b_side(i):
            co, t = bufs[i % n_buf]
            return [[m.minmax_magnitude(ctx, co, t, der, dimensions=[d])[0] for d in range(3)] for der in (1, 2)]

        def a_va(i):
            return m.minmax_axes(ctx, *bufs[i % n_buf], 1, 2, want_trajectory=False)

        def a_all(i):
            return m.minmax_axes(ctx, *bufs[i % n_buf], 0, 5, want_trajectory=False)

        a, b = a_va(0).segment, b_side(0)
        ctx.sync()
        worst = 0.0                                             # the two sides answer the same question: max(|min|, |max|) per axis
        for j in range(2):
            for d in range(3):
                got = torch.maximum(a[:, :, d, j, 1].abs(), a[:, :, d, j, 3].abs())
                want = b[j][d][:, :, 3]
                worst = max(worst, float(((got - want).abs() / want.abs().clamp(min=1.0)).max()))
        assert worst <= 1e-9, worst

        sides = {"a_va": a_va, "a_all": a_all, "b": b_side}
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
        plan.close()
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    spread = 100.0 * (max(runs["b"]) - min(runs["b"])) / med["b"]
    roofline_us = B * K * D * N * 8 / 8e12 * 1e6                # the coefficient read at 8 TB/s
    out = {"tool": "bench_axis_minmax", "N": N, "K": K, "D": D, "batch": B, "calls": args.calls, "repeats": args.repeats, "buffers": n_buf,
           "A_velocity_acceleration_us": round(med["a_va"], 1), "A_position_to_snap_us": round(med["a_all"], 1), "B_six_magnitude_calls_us": round(med["b"], 1),
           "B_spread_percent": round(spread, 2), "A_velocity_acceleration_runs_us": [round(x, 1) for x in runs["a_va"]],
           "A_position_to_snap_runs_us": [round(x, 1) for x in runs["a_all"]], "B_runs_us": [round(x, 1) for x in runs["b"]],
           "A_vs_B_largest_relative_difference": worst,
           "A_lt_B_met": bool(med["a_va"] < (1.0 - spread / 100.0) * med["b"]),
           "A_position_to_snap_lt_B_met": bool(med["a_all"] < (1.0 - spread / 100.0) * med["b"]),
           "coefficient_read_roofline_us": round(roofline_us, 2)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
