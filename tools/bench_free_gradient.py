"""Device time of the batched gradient with respect to the free derivatives (A: one mtg_free_gradient call with grad_coeffs only;
A2: the same call with coeffs as well, i.e. with the derivative cost's gradient added on the fly) against what the library offered
before for the same numbers (B): n_free update_from_free calls with d_fixed = 0 and unit d_free columns, which build
J = d coeffs / d d_free for the batch's times, then one torch.einsum with G; all of it timed.  B goes through the forward kernels:
A must agree with it within 1e-9 of the largest entry (asserted).  Required: A < B.  `collision`: collision_cost with its gradient
on the same batch (the distance-field tools' 256^3 field), for scale.

Workload: 10k x K = 8 x N = 10 x D = 3, d = 4, the standard plan (n_free = 28).  Protocol of tools/bench_collision_cost.py: one
process; device events around `--calls` back-to-back calls after a warm-up; the inputs rotate over enough buffers that they come
from HBM (more than 512 MB of them); the sides alternate, the round is repeated `--repeats` times, the spread over the repeats is
reported with the median.  A is timed twice: through Plan.free_gradient (which allocates its outputs) and through the C entry
with preallocated outputs (`a_raw`); back-to-back call times are bounded below by the host's enqueue cost, which for a kernel of
a few microseconds is what they measure.  Recorded, not gated: a_raw's share of the 8 TB/s roofline by the byte count
8 (K + K D N (1 or 2) + D n_free) per trajectory.  With --remarks <dir of a MTG_BUILD_REMARKS build>: VGPRs, scratch and LDS of
every instantiation (no scratch: asserted).  Asserted too: the call equals the host form bit for bit on the first trajectories.
Prints one JSON line; --out appends it to a file.

    python tools/bench_free_gradient.py [--batch 10000] [--calls 200] [--repeats 5] [--remarks DIR] [--out profiles/free_gradient_bench.jsonl]
"""
import argparse
import ctypes
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import mav_trajectory_generation_amd as m  # noqa: E402
from bench_distance_field import spheres_field, timed  # noqa: E402


def resources(remarks):
    """{N: {vgprs, agprs, scratch, lds}} of the kernel's instantiations, from the build's resource remarks."""
    text = open(os.path.join(remarks, "mtg_pullback.log")).read()
    out = {}
    for name, body in re.findall(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", text, flags=re.S):
        inst = re.search(r"free_gradient_kernelILi(\d+)E", name)
        if not inst:
            continue
        get = lambda key: int(re.search(re.escape(key) + r": (\d+)", body).group(1))
        out[f"N{inst.group(1)}"] = {"vgprs": get("VGPRs"), "agprs": get("AGPRs"), "scratch": get("ScratchSize [bytes/lane]"),
                                    "lds": get("LDS Size [bytes/block]")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=10_000)
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--calls-b", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-collision", action="store_true", help="skip the collision cost call recorded for scale")
    ap.add_argument("--remarks", default=None, help="directory of a MTG_BUILD_REMARKS build: resources per instantiation")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, K, D, B, d = 10, args.segments, 3, args.batch, 4
    res = resources(args.remarks) if args.remarks else None
    if res is not None:
        assert len(res) == 6 and all(r["scratch"] == 0 for r in res.values()), res
    ctx = m.Context(0)
    with torch.cuda.stream(ctx.stream):
        masks = m.ends_full_masks(N, K)
        plan = m.Plan(ctx, N, D, K, d, masks)
        n_free, n_fixed = plan.n_free, plan.n_fixed
        per_buffer = B * K * D * N * 8
        n_buf = max(2, (512 << 20) // per_buffer + 1)
        gen = torch.Generator(device="cuda").manual_seed(2026)
        bufs = []
        for i in range(n_buf):
            t, f = m.random_waypoint_batch(B, K, D, N, masks, seed=8 + i, device="cuda", box=10.0)
            co, _, _ = plan.solve(t, f)
            G = torch.randn((B, K, D, N), dtype=torch.float64, device="cuda", generator=gen)
            bufs.append((t.clone(), G, co.clone()))
        ctx.sync()
        lay = plan.layout(B, "aos")
        out_free = torch.empty((B, D, n_free), dtype=torch.float64, device="cuda")
        zeros_fixed = torch.zeros((B, D, n_fixed), dtype=torch.float64, device="cuda")
        units = [torch.zeros((B, D, n_free), dtype=torch.float64, device="cuda") for _ in range(n_free)]
        for j, u in enumerate(units):
            u[:, :, j] = 1.0
        p = lambda x: ctypes.c_void_p(0) if x is None else ctypes.c_void_p(x.data_ptr())

        def a_raw(i, with_coeffs=False):
            t, G, co = bufs[i % n_buf]
            rc = ctx.lib.mtg_free_gradient(plan.handle, B, ctypes.byref(lay), p(t), p(G), p(co if with_coeffs else None), 1.0, p(out_free), None)
            assert rc == 0
            return out_free

        def side_b(i):
            t, G, _ = bufs[i % n_buf]
            J = torch.stack([plan.update_from_free(t, zeros_fixed, u)[0] for u in units])      # [n_free][B][K][D][N]
            return torch.einsum("jbkdi,bkdi->bdj", J, G)

        sides = {"a": lambda i: plan.free_gradient(bufs[i % n_buf][0], bufs[i % n_buf][1])[0],
                 "a_raw": a_raw,
                 "a2": lambda i: plan.free_gradient(*bufs[i % n_buf], 1.0)[0],
                 "a2_raw": lambda i: a_raw(i, True),
                 "b": side_b}
        if not args.no_collision:
            box, margin = 10.0, 1.0
            rng = np.random.default_rng(2025)
            centres, radii = rng.uniform(-box, box, (16, 3)), rng.uniform(0.5, 1.5, 16)
            lo, h = -(box + margin), 2.0 * (box + margin) / 255.0
            field = m.DistanceField(spheres_field((256, 256, 256), (lo, lo, lo), h, centres, radii), (lo, lo, lo), h)
            sides["collision"] = lambda i: m.collision_cost(ctx, bufs[i % n_buf][2], bufs[i % n_buf][0], field, 0.01, inflation=0.2,
                                                            epsilon=0.5, speed_epsilon=1e-3, max_samples=1 << 16)

        # A against the host form (bit for bit, first trajectories) and against B (the forward kernels: 1e-9 of the largest entry)
        t0, G0, c0 = bufs[0]
        got = {name: sides[name](0).clone() for name in ("a", "a_raw", "a2", "a2_raw")}
        via_b = side_b(0)
        ctx.sync()
        assert torch.equal(got["a"], got["a_raw"]) and torch.equal(got["a2"], got["a2_raw"])
        nb = min(32, B)
        h1, _ = m.free_gradient_host(N, d, masks, t0[:nb].cpu().numpy(), G0[:nb].cpu().numpy())
        h2, _ = m.free_gradient_host(N, d, masks, t0[:nb].cpu().numpy(), G0[:nb].cpu().numpy(), c0[:nb].cpu().numpy(), 1.0)
        same = bool(np.array_equal(h1, got["a"][:nb].cpu().numpy()) and np.array_equal(h2, got["a2"][:nb].cpu().numpy()))
        assert same
        a_vs_b = float((got["a"] - via_b).abs().max() / via_b.abs().max())
        assert a_vs_b <= 1e-9, a_vs_b

        for name, fn in sides.items():
            timed(ctx, fn, 1 if name in ("b", "collision") else args.warmup)
        runs = {k: [] for k in sides}
        for _ in range(args.repeats):
            for name, fn in sides.items():
                runs[name].append(timed(ctx, fn, args.calls_b if name in ("b", "collision") else args.calls))
        plan.close()
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    spread = {k: round(100.0 * (max(v) - min(v)) / med[k], 2) for k, v in runs.items()}
    assert med["a"] < med["b"] and med["a_raw"] < med["b"], med
    bytes_a = 8 * (K + K * D * N + D * n_free) * B
    bytes_a2 = 8 * (K + 2 * K * D * N + D * n_free) * B
    roof = lambda nbytes: nbytes / 8e12 * 1e6      # microseconds at 8 TB/s
    out = {"tool": "bench_free_gradient", "N": N, "K": K, "D": D, "d": d, "batch": B, "n_free": n_free, "calls": args.calls,
           "calls_b": args.calls_b, "repeats": args.repeats, "buffers": n_buf, "us": {k: round(v, 2) for k, v in med.items()},
           "b_over_a": round(med["b"] / med["a"], 1), "b_over_a_raw": round(med["b"] / med["a_raw"], 1),
           "a_vs_b_over_largest": a_vs_b, "device_equals_host_bitwise": same,
           "bytes": {"a": bytes_a, "a2": bytes_a2}, "roofline_us_8TBs": {"a": round(roof(bytes_a), 2), "a2": round(roof(bytes_a2), 2)},
           "share_of_roofline": {"a_raw": round(roof(bytes_a) / med["a_raw"], 3), "a2_raw": round(roof(bytes_a2) / med["a2_raw"], 3)},
           "spread_percent": spread, "runs_us": {k: [round(x, 2) for x in v] for k, v in runs.items()}, "resources": res}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
