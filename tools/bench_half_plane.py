"""Device time of the batched half-plane feasibility check (A) against what the library offered before it for an axis-aligned box
about the origin (B = three minmax_magnitude calls, derivative 0, one dimension each, plus the tensor comparison).

Protocol of tools/bench_feasibility.py: one process; device events around `--calls` back-to-back calls after a warm-up; the inputs
rotate over enough coefficient buffers that they come from HBM (more than the 256 MB last-level cache); A and B alternate and
the round is repeated `--repeats` times: s = spread of B over the repeats, A (box) < B counts as met at A < (1 - s / 100) B.
A is timed twice: a shared bounding box (six planes, three root searches: the (+e, -e) pairs reuse their critical points) and
a shared set of six oblique planes (six searches).  Prints one JSON line; --out appends it to a file.

    python tools/bench_half_plane.py [--batch 10000] [--calls 100] [--repeats 5] [--out profiles/half_plane_bench.jsonl]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
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
    ap.add_argument("--edge", type=float, default=24.0)
    ap.add_argument("--only", choices=["a_box", "a_oblique", "b"], default=None, help="one side only, once (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, K, D, B = 10, args.segments, 3, args.batch
    ctx = m.Context(0)
    with torch.cuda.stream(ctx.stream):
        masks = m.ends_full_masks(N, K)
        plan = m.Plan(ctx, N, D, K, N // 2 - 1, masks)
        per_buffer = B * K * D * N * 8
        n_buf = max(2, (512 << 20) // per_buffer + 1)          # twice the last-level cache
        bufs = []
        for i in range(n_buf):
            t, f = m.random_waypoint_batch(B, K, D, N, masks, seed=8 + i, device="cuda")
            co, _, _ = plan.solve(t, f)
            bufs.append((co.clone(), t.clone()))
        ctx.sync()
        half = args.edge / 2.0
        box = torch.from_numpy(m.bounding_box_half_planes([0.0, 0.0, 0.0], [args.edge] * 3)).cuda()
        nrm = np.random.default_rng(3).standard_normal((6, 3))
        nrm /= np.sqrt((nrm * nrm).sum(axis=1, keepdims=True))
        oblique = torch.from_numpy(m.half_planes(-half * nrm, nrm)).cuda()

        def b_side(i):
            co, t = bufs[i % n_buf]
            ok = None
            for d in range(3):
                traj = m.minmax_magnitude(ctx, co, t, 0, dimensions=[d])[1]
                inside = traj[:, 3] < half
                ok = inside if ok is None else ok & inside
            return ok

        a_box = m.check_half_plane_feasibility(ctx, *bufs[0], box)
        a_obl = m.check_half_plane_feasibility(ctx, *bufs[0], oblique)
        b_ok = b_side(0)
        ctx.sync()
        assert bool((a_box.trajectory_feasible.bool() == b_ok).all())           # the two sides answer the same question
        mix = {"box": int(a_box.trajectory_feasible.sum()), "oblique": int(a_obl.trajectory_feasible.sum()), "of": B}

        sides = {"a_box": lambda i: m.check_half_plane_feasibility(ctx, *bufs[i % n_buf], box),
                 "a_oblique": lambda i: m.check_half_plane_feasibility(ctx, *bufs[i % n_buf], oblique), "b": b_side}
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
    out = {"tool": "bench_half_plane", "N": N, "K": K, "D": D, "batch": B, "calls": args.calls, "repeats": args.repeats,
           "buffers": n_buf, "box_edge": args.edge, "A_box_us": round(med["a_box"], 1), "A_oblique6_us": round(med["a_oblique"], 1),
           "B_us": round(med["b"], 1), "B_spread_percent": round(spread, 2), "A_box_runs_us": [round(x, 1) for x in runs["a_box"]],
           "A_oblique6_runs_us": [round(x, 1) for x in runs["a_oblique"]], "B_runs_us": [round(x, 1) for x in runs["b"]],
           "feasible": mix, "A_box_lt_B_met": bool(med["a_box"] < (1.0 - spread / 100.0) * med["b"]),
           "coefficient_read_roofline_us": round(roofline_us, 2),
           "A_box_share_of_roofline_percent": round(100.0 * roofline_us / med["a_box"], 1),
           "M_trajectories_per_s_A_box": round(B / med["a_box"], 2)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
