"""Device time of one batched time-objective call (A = mtg_time_objective: solve with cost, ONE maxima-only search launch over
both constrained derivatives, one finishing launch) against what the library offered before it for the same numbers (B =
Plan.solve(want_cost=True) + minmax_magnitude for derivative 1 + minmax_magnitude for derivative 2 + the torch arithmetic that
forms cost_time, the soft terms and the total).

One process; device events around `--calls` back-to-back calls after a warm-up; inputs and coefficient outputs rotate over
enough buffer sets that the searches read their coefficients from HBM (more than twice the 256 MB last-level cache); A and B
alternate and the pair is repeated `--repeats` times: s = spread of B over the repeats, the expectation A <= B counts as met at
A < (1 - s / 100) B (A wins by more than B's own spread).  Before timing, A's total is compared with B's on one buffer set.
--resources: a kernel-resource-usage log of csrc/mtg_objective.hip (the build writes one per translation unit with
MTG_BUILD_REMARKS=<dir>); the search kernel's registers, scratch and occupancy are added to the line.
Prints one JSON line; --out appends it to a file.

    python tools/bench_time_objective.py [--batch 10000] [--calls 100] [--repeats 5] [--out profiles/time_objective_bench.jsonl]
"""
import argparse
import json
import os
import re
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


def kernel_resources(path, n_coeffs, dim_c):
    """VGPRs, AGPRs, scratch, occupancy of mtg_objective_seg_kernel<n_coeffs, dim_c> from a -Rpass-analysis=kernel-resource-usage log."""
    want = f"mtg_objective_seg_kernelILi{n_coeffs}ELi{dim_c}EE"
    out, inside = {}, False
    for line in open(path):
        if "Function Name:" in line:
            inside = want in line
        elif inside:
            for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                             ("waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)"), ("sgprs", r" SGPRs: (\d+)")):
                hit = re.search(pat, line)
                if hit and key not in out:
                    out[key] = int(hit.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=10_000)
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["a", "b"], default=None, help="one side only, once (for a kernel trace)")
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, K, D, B = 10, args.segments, 3, args.batch
    v_max, a_max = 3.0, 5.0
    params = m.TimeObjectiveParams(time_cost_kind=m.TimeCostKind.kSquaredTime, constraints=[(1, v_max), (2, a_max)])
    ctx = m.Context(0)
    with torch.cuda.stream(ctx.stream):
        masks = m.ends_full_masks(N, K)
        plan = m.Plan(ctx, N, D, K, N // 2 - 1, masks)
        per_buffer = B * K * D * N * 8
        n_buf = max(2, (512 << 20) // per_buffer + 1)          # twice the last-level cache
        sets = []
        for i in range(n_buf):
            t, f = m.random_waypoint_batch(B, K, D, N, masks, seed=8 + i, device="cuda")
            sets.append((t.clone(), f.clone(), torch.empty((B, K, D, N), dtype=torch.float64, device="cuda")))
        ctx.sync()

        def a(i):
            t, f, co = sets[i % n_buf]
            return m.time_objective(plan, t, f, params, coeffs=co)

        def b(i):
            t, f, co = sets[i % n_buf]
            _, _, cost = plan.solve(t, f, want_cost=True, coeffs=co)
            _, tv, _ = m.minmax_magnitude(ctx, co, t, 1)
            _, ta, _ = m.minmax_magnitude(ctx, co, t, 2)
            total_time = t.sum(dim=1)
            soft = (torch.clamp(torch.exp((tv[:, 3] - v_max) / v_max * params.soft_constraint_weight), max=params.maximum_cost)
                    + torch.clamp(torch.exp((ta[:, 3] - a_max) / a_max * params.soft_constraint_weight), max=params.maximum_cost))
            return cost + total_time * total_time * params.time_penalty + soft

        ra, rb = a(0).objective.clone(), b(0).clone()
        ctx.sync()
        agree = float(((ra - rb).abs() / rb.abs()).max())
        assert agree <= 1e-9, agree
        sides = {"a": a, "b": b}
        if args.only:
            us = timed(ctx, sides[args.only], args.calls)
            print(json.dumps({"only": args.only, "us": round(us, 1), "calls": args.calls}))
            plan.close()
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
    out = {"tool": "bench_time_objective", "N": N, "K": K, "D": D, "batch": B, "constraints": [[1, v_max], [2, a_max]],
           "calls": args.calls, "repeats": args.repeats, "buffer_sets": n_buf, "A_us": round(med["a"], 1), "B_us": round(med["b"], 1),
           "A_spread_percent": round(100.0 * (max(runs["a"]) - min(runs["a"])) / med["a"], 2), "B_spread_percent": round(spread, 2),
           "A_runs_us": [round(x, 1) for x in runs["a"]], "B_runs_us": [round(x, 1) for x in runs["b"]],
           "A_below_B_by_more_than_B_spread": bool(med["a"] < (1.0 - spread / 100.0) * med["b"]),
           "A_vs_B_max_relative_difference": agree, "M_objectives_per_s_A": round(B / med["a"], 2),
           "search_kernel_lds_bytes_per_workgroup": 64 * 2 * (2 * N - 5) * 8}
    if args.resources:
        out["search_kernel"] = kernel_resources(args.resources, N, 3)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
