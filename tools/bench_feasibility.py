"""Device time of the batched input-feasibility check (A) against what the library offered before it for the same three root
searches (B = minmax_magnitude with derivative 1, 2 and 3 on the same batch, summed).

One process; device events around `--calls` back-to-back calls after a warm-up; the inputs rotate over enough coefficient
buffers that they come from HBM (more than the 256 MB last-level cache); A and B alternate and the pair is repeated `--repeats`
times: s = spread of B over the repeats, the expectation A <= B counts as met at A <= (1 + s / 100) B.
Two limit sets for A, both with f_min, f_max, v_max and omega_xy_max: the reference's defaults, and a loose one under which every
trajectory is feasible.  Prints one JSON line; --out appends it to a file.

    python tools/bench_feasibility.py [--batch 10000] [--calls 100] [--repeats 5] [--out profiles/feasibility.jsonl]
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
    ap.add_argument("--only", choices=["a_defaults", "a_loose", "b"], default=None, help="one side only, once (for a kernel trace)")
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
        limit_sets = {
            "a_defaults": m.InputConstraints(f_min=0.5 * 9.81, f_max=1.5 * 9.81, v_max=3.0, omega_xy_max=1.5707963267948966),
            "a_loose": m.InputConstraints(f_min=1e-3, f_max=1e6, v_max=1e6, omega_xy_max=1e6),
        }
        mix = {}
        for name, c in limit_sets.items():
            traj = m.check_input_feasibility(ctx, bufs[0][0], bufs[0][1], c)[0]
            ctx.sync()
            codes, counts = torch.unique(traj, return_counts=True)
            mix[name] = {int(k): int(v) for k, v in zip(codes.cpu(), counts.cpu())}
        assert set(mix["a_loose"]) == {0}, mix["a_loose"]       # no check is skipped and none fails

        def a(c):
            return lambda i: m.check_input_feasibility(ctx, *bufs[i % n_buf], c)

        def b_der(der):
            return lambda i: m.minmax_magnitude(ctx, *bufs[i % n_buf], der)

        sides = {"a_defaults": [a(limit_sets["a_defaults"])], "a_loose": [a(limit_sets["a_loose"])], "b": [b_der(1), b_der(2), b_der(3)]}
        if args.only:
            us = sum(timed(ctx, fn, args.calls) for fn in sides[args.only])
            print(json.dumps({"only": args.only, "us": round(us, 1), "calls": args.calls}))
            return
        for fns in sides.values():
            for fn in fns:
                timed(ctx, fn, args.warmup)
        runs = {k: [] for k in sides}
        b_parts = []
        for _ in range(args.repeats):
            for name, fns in sides.items():
                parts = [timed(ctx, fn, args.calls) for fn in fns]
                runs[name].append(sum(parts))
                if name == "b":
                    b_parts.append(parts)
        plan.close()
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    spread = 100.0 * (max(runs["b"]) - min(runs["b"])) / med["b"]
    out = {"tool": "bench_feasibility", "N": N, "K": K, "D": D, "batch": B, "calls": args.calls, "repeats": args.repeats,
           "buffers": n_buf, "A_defaults_us": round(med["a_defaults"], 1), "A_all_feasible_us": round(med["a_loose"], 1),
           "B_us": round(med["b"], 1), "B_parts_us_der123": [round(x, 1) for x in b_parts[len(b_parts) // 2]],
           "B_spread_percent": round(spread, 2), "A_runs_us": [round(x, 1) for x in runs["a_loose"]],
           "B_runs_us": [round(x, 1) for x in runs["b"]], "verdict_mix": mix,
           "A_le_B_met": bool(med["a_loose"] <= (1.0 + spread / 100.0) * med["b"]),
           "M_trajectories_per_s_A": round(B / med["a_loose"], 2)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
