"""Device time of the CERTIFIED distance-field check (A: one certify_distance_field call with the defaults, min_depth 4, max_depth
16, max_frontier 1024, the Lipschitz constant from DistanceField.lipschitz_bound()) against the sampled check at the benchmark's
spacing (B: one check_distance_field call at dt = 0.01) in the same run.  Recorded, not gated: no ratio is promised.

Protocol of tools/bench_distance_field.py, whose batches and field these are: one process; device events around `--calls`
back-to-back calls after a warm-up; the inputs rotate over enough coefficient buffers that they come from HBM (more than 512 MB of
them); the sides alternate and the round is repeated `--repeats` times, the spread over the repeats is reported with the median.
The field: 256^3 float32 (64 MiB) of 16 spheres in the waypoint box, trilinear, outside_distance 0.  Next to the times: the nodes
per segment of A (mean and maximum) and the samples per segment of B, the verdict counts of both calls, the trajectories that B
passes and A proves colliding (and the reverse, which must not exist), and -- with --remarks <dir of a MTG_BUILD_REMARKS build> --
VGPRs, scratch and LDS of every instantiation.  Asserted: A equals the host form bit for bit on the first trajectories, no FREE
trajectory fails B, and no instantiation uses scratch.  Prints one JSON line; --out appends it to a file.

    python tools/bench_certify_distance_field.py [--batch 10000] [--calls 100] [--repeats 5] [--remarks DIR] [--out profiles/certify_distance_field_bench.jsonl]
"""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import torch  # noqa: E402
import mav_trajectory_generation_amd as m  # noqa: E402
from bench_distance_field import spheres_field, timed  # noqa: E402


def resources(remarks):
    """{instantiation: {vgprs, scratch, lds}} of the segment kernels, from the build's resource remarks."""
    text = open(os.path.join(remarks, "mtg_certify.log")).read()
    out = {}
    for name, body in re.findall(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", text, flags=re.S):
        inst = re.search(r"certify_seg_kernelILi(\d+)E", name)
        if not inst:
            continue
        get = lambda key: int(re.search(re.escape(key) + r": (\d+)", body).group(1))
        out[f"N{inst.group(1)}"] = {"vgprs": get("VGPRs"), "scratch": get("ScratchSize [bytes/lane]"), "lds": get("LDS Size [bytes/block]")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=10_000)
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--spheres", type=int, default=16)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--remarks", default=None, help="directory of a MTG_BUILD_REMARKS build: resources per instantiation")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, K, D, B, M = 10, args.segments, 3, args.batch, args.spheres
    box, margin, inflation = 10.0, 1.0, 0.2                     # random_waypoint_batch's box
    rng = np.random.default_rng(2025)
    centres, radii = rng.uniform(-box, box, (M, 3)), rng.uniform(0.5, 1.5, M)
    res = resources(args.remarks) if args.remarks else None
    if res is not None:
        assert len(res) == 5 and all(r["scratch"] == 0 for r in res.values()), res
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
        span = 2.0 * (box + margin)
        h = span / 255.0
        lo = -(box + margin)
        field = m.DistanceField(spheres_field((256, 256, 256), (lo, lo, lo), h, centres, radii), (lo, lo, lo), h)
        lipschitz = field.lipschitz_bound()

        certify = lambda i: m.certify_distance_field(ctx, *bufs[i % n_buf], field, lipschitz, inflation=inflation)
        sampled = lambda i: m.check_distance_field(ctx, *bufs[i % n_buf], field, args.dt, inflation=inflation, max_samples=1 << 16)
        sides = {"a": certify, "b": sampled}

        a, b = certify(0), sampled(0)
        ctx.sync()
        nb = min(64, B)
        co, t = bufs[0][0][:nb].cpu().numpy(), bufs[0][1][:nb].cpu().numpy()
        host = m.certify_distance_field_host(co, t, m.DistanceField(field.distances.cpu().numpy(), field.origin, h), lipschitz, inflation=inflation)
        for name, x, y in zip(a._fields[:11], a, host):
            assert x[:nb].cpu().numpy().tobytes() == y.tobytes(), name
        codes = torch.bincount(a.trajectory_result, minlength=4).tolist()
        seg_codes = torch.bincount(a.segment_result.view(-1), minlength=4).tolist()
        b_pass = b.trajectory_feasible == 1
        assert not bool((~b_pass & (a.trajectory_result == 1)).any()), "a FREE trajectory fails a sample of the sampled check"
        nodes, samples = a.segment_nodes.double(), b.segment_samples.double()
        stats = {"lipschitz": lipschitz, "nodes_per_segment_mean": round(float(nodes.mean()), 2), "nodes_per_segment_max": int(nodes.max()),
                 "depth_max": int(a.segment_depth.max()), "samples_per_segment_mean": round(float(samples.mean()), 1),
                 "samples_per_segment_max": int(samples.max()),
                 "a_trajectories": dict(zip(("collides", "free", "undecided_depth", "undecided_budget"), codes)),
                 "a_segments": dict(zip(("collides", "free", "undecided_depth", "undecided_budget"), seg_codes)),
                 "b_trajectories": {"feasible": int(b_pass.sum()), "infeasible": int((~b_pass).sum())},
                 "b_passes_a_collides": int((b_pass & (a.trajectory_result == 0)).sum()),
                 "b_passes_a_undecided": int((b_pass & (a.trajectory_result >= 2)).sum()),
                 "b_fails_a_free": int((~b_pass & (a.trajectory_result == 1)).sum())}

        for name, fn in sides.items():
            timed(ctx, fn, args.warmup)
        runs = {k: [] for k in sides}
        for _ in range(args.repeats):
            for name, fn in sides.items():
                runs[name].append(timed(ctx, fn, args.calls))
        plan.close()
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    spread = {k: round(100.0 * (max(v) - min(v)) / med[k], 2) for k, v in runs.items()}
    out = {"tool": "bench_certify_distance_field", "N": N, "K": K, "D": D, "batch": B, "spheres": M, "dt": args.dt, "inflation": inflation,
           "min_depth": 4, "max_depth": 16, "max_frontier": 1024, "calls": args.calls, "repeats": args.repeats, "buffers": n_buf,
           "field": [256, 256, 256], "field_mib": 64, **stats, "us": {k: round(v, 1) for k, v in med.items()},
           "a_over_b": round(med["a"] / med["b"], 3), "spread_percent": spread,
           "runs_us": {k: [round(x, 1) for x in v] for k, v in runs.items()}, "resources": res}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
