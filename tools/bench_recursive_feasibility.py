"""Device time of the batched recursive input-feasibility check (A = check_input_feasibility_recursive) against the analytic
check (B = check_input_feasibility) on the same inputs and limits.

The workload of tools/bench_feasibility.py: 10k trajectories x K = 8 x N = 10 x D = 3; one process; device events around
`--calls` back-to-back calls after a warm-up; the inputs rotate over enough coefficient buffers that they come from HBM (more
than the 256 MB last-level cache); A and B alternate and the round is repeated `--repeats` times.  Two limit sets, both with
f_min, f_max, v_max and omega_xy_max: a loose one that nobody fails, and the reference's defaults.  s = spread of B over the
repeats; "A below B" counts as met at A < (1 - s / 100) B.  The figure is a report, not a gate.  Prints one JSON line; --out
appends it to a file.

    python tools/bench_recursive_feasibility.py [--batch 10000] [--calls 100] [--repeats 5] [--out profiles/recursive_feasibility_bench.jsonl]
    rocprofv3 --kernel-trace --stats -- python tools/bench_recursive_feasibility.py --only a_loose     (kernel time, in a run of its own)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import mav_trajectory_generation_amd as m  # noqa: E402

from bench_feasibility import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=10_000)
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["a_loose", "a_defaults", "b_loose", "b_defaults"], default=None,
                    help="one side only, once (for a kernel trace)")
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
            "loose": m.InputConstraints(f_min=1e-3, f_max=1e6, v_max=1e6, omega_xy_max=1e6),
            "defaults": m.InputConstraints(f_min=0.5 * 9.81, f_max=1.5 * 9.81, v_max=3.0, omega_xy_max=1.5707963267948966),
        }
        checks = {"a": m.check_input_feasibility_recursive, "b": m.check_input_feasibility}
        mix, sections = {}, {}
        for side, check in checks.items():
            for name, c in limit_sets.items():
                traj = check(ctx, bufs[0][0], bufs[0][1], c)[0]
                ctx.sync()
                codes, counts = torch.unique(traj, return_counts=True)
                mix[f"{side}_{name}"] = {int(k): int(v) for k, v in zip(codes.cpu(), counts.cpu())}
        for name, c in limit_sets.items():
            sec = m.check_input_feasibility_recursive(ctx, bufs[0][0], bufs[0][1], c, want_sections=True)[4]
            ctx.sync()
            sections[name] = {"mean": round(float(sec.double().mean()), 3), "max": int(sec.max())}

        def side_fn(check, c):
            return lambda i: check(ctx, *bufs[i % n_buf], c, want_segments=True, want_bounds=True)

        sides = {f"{side}_{name}": side_fn(check, c) for side, check in checks.items() for name, c in limit_sets.items()}
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
    spread = {k: 100.0 * (max(runs[k]) - min(runs[k])) / med[k] for k in ("b_loose", "b_defaults")}
    out = {"tool": "bench_recursive_feasibility", "N": N, "K": K, "D": D, "batch": B, "calls": args.calls, "repeats": args.repeats,
           "buffers": n_buf,
           "A_all_feasible_us": round(med["a_loose"], 1), "B_all_feasible_us": round(med["b_loose"], 1),
           "B_all_feasible_spread_percent": round(spread["b_loose"], 2),
           "A_defaults_us": round(med["a_defaults"], 1), "B_defaults_us": round(med["b_defaults"], 1),
           "B_defaults_spread_percent": round(spread["b_defaults"], 2),
           "runs_us": {k: [round(x, 1) for x in v] for k, v in runs.items()}, "verdict_mix": mix, "sections_per_segment": sections,
           "A_below_B_all_feasible": bool(med["a_loose"] < (1.0 - spread["b_loose"] / 100.0) * med["b_loose"]),
           "A_below_B_defaults": bool(med["a_defaults"] < (1.0 - spread["b_defaults"] / 100.0) * med["b_defaults"]),
           "M_trajectories_per_s_A_all_feasible": round(B / med["a_loose"], 2)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
