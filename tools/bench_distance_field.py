"""Device time of the batched distance-field clearance check (A) against what the library offered before for the same question
(B): sample_range(n_derivatives=1) over the longest trajectory, then index arithmetic, eight gathers, trilinear interpolation and a
per-trajectory minimum as torch operations.  B samples on the trajectory's global time grid, so it looks at about as many samples,
not at the same ones: it is a timing comparator only.  Recorded, not gated.

Protocol of tools/bench_keep_out_zones.py: one process; device events around `--calls` back-to-back calls after a warm-up; the
inputs rotate over enough coefficient buffers that they come from HBM (more than 512 MB of them); the sides alternate and the round
is repeated `--repeats` times, the spread over the repeats is reported with the median.  Sides: a -- one check_distance_field call,
dt = 0.01, trilinear, a 256^3 float32 field (64 MiB) of 16 spheres in the waypoint box; a_lanes1 / 4 / 16 / 64 -- the same under the
measurement knob "field_lanes"; a_nearest; a_big -- the same spheres on a 512 x 512 x 320 field (320 MiB, finer voxels over the
same box: beyond the last-level cache); b -- the comparator (`--calls-b` calls).  Next to the times: the mean number of samples per
segment, the share of the comparator's samples that fall outside the grid, and -- with --remarks <dir of a MTG_BUILD_REMARKS
build> -- VGPRs, scratch and LDS of every instantiation.  Asserted: the default call equals the host form on the first
trajectories in every integer output, all five group sizes give the same bits, and no instantiation uses scratch.  Prints one JSON
line; --out appends it to a file.

    python tools/bench_distance_field.py [--batch 10000] [--calls 100] [--repeats 5] [--sides a,b] [--remarks DIR] [--out profiles/distance_field_bench.jsonl]
"""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import mav_trajectory_generation_amd as m  # noqa: E402

torch.set_num_threads(min(16, torch.get_num_threads()))


def timed(ctx, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(ctx.stream)
    for i in range(calls):
        fn(i)
    e1.record(ctx.stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def resources(remarks):
    """{instantiation: {vgprs, scratch, lds}} of the segment kernels, from the build's resource remarks."""
    text = open(os.path.join(remarks, "mtg_field.log")).read()
    out = {}
    for name, body in re.findall(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", text, flags=re.S):
        inst = re.search(r"seg_kernelILi(\d+)ELi(\d+)E", name)
        if not inst:
            continue
        get = lambda key: int(re.search(re.escape(key) + r": (\d+)", body).group(1))
        out[f"N{inst.group(1)}_G{inst.group(2)}"] = {"vgprs": get("VGPRs"), "scratch": get("ScratchSize [bytes/lane]"),
                                                     "lds": get("LDS Size [bytes/block]")}
    return out


def spheres_field(dims, origin, h, centres, radii):
    """float32 [nz][ny][nx] on the device: distance to the nearest sphere's surface at the voxel centres, a z-slab at a time."""
    nx, ny, nz = dims
    x = origin[0] + h * torch.arange(nx, device="cuda", dtype=torch.float64)
    y = origin[1] + h * torch.arange(ny, device="cuda", dtype=torch.float64)
    out = torch.empty((nz, ny, nx), dtype=torch.float32, device="cuda")
    for iz in range(nz):
        z = origin[2] + h * iz
        d = None
        for c, r in zip(centres, radii):
            e = torch.sqrt((x[None, :] - c[0]) ** 2 + (y[:, None] - c[1]) ** 2 + (z - c[2]) ** 2) - r
            d = e if d is None else torch.minimum(d, e)
        out[iz] = d.to(torch.float32)
    return out


class Comparator:
    """B: positions from sample_range, then the lookup and the minimum as tensor operations."""

    def __init__(self, ctx, field, dt, n_samples, inflation):
        self.ctx, self.field, self.dt, self.n_samples, self.inflation = ctx, field, dt, n_samples, inflation
        nz, ny, nx = field.distances.shape
        self.flat = field.distances.view(-1)
        self.origin = torch.tensor(field.origin, dtype=torch.float64, device="cuda")
        self.top = torch.tensor([nx - 1, ny - 1, nz - 1], dtype=torch.float64, device="cuda")
        self.stride = (1, nx, nx * ny)
        self.r = 1.0 / field.voxel_size
        self.outside_share = None

    def __call__(self, coeffs, times):
        pos = m.sample_range(self.ctx, coeffs, times, 0.0, self.dt, self.n_samples, n_derivatives=1)[:, :, 0, :]   # [B][S][3]
        u = (pos - self.origin) * self.r
        inside = ((u >= 0) & (u <= self.top)).all(dim=-1)
        cell = torch.minimum(u.floor().clamp_(min=0.0), self.top - 1)
        f = u - cell
        cell = cell.long()
        base = cell[..., 0] + cell[..., 1] * self.stride[1] + cell[..., 2] * self.stride[2]
        v = [self.flat[base + (dx + dy * self.stride[1] + dz * self.stride[2])].double() for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
        fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
        x00, x10, x01, x11 = (torch.addcmul(v[j], fx, v[j + 1] - v[j]) for j in (0, 2, 4, 6))
        y0, y1 = torch.addcmul(x00, fy, x10 - x00), torch.addcmul(x01, fy, x11 - x01)
        d = torch.addcmul(y0, fz, y1 - y0)
        d = torch.where(inside, d, torch.full_like(d, self.field.outside_distance))
        clearance = d.amin(dim=1) - self.inflation
        if self.outside_share is None:
            self.outside_share = float((~inside).double().mean())
        return clearance > 0.0, clearance


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=10_000)
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--spheres", type=int, default=16)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--calls-b", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sides", default="a,a_lanes1,a_lanes4,a_lanes16,a_lanes64,a_nearest,a_big,b")
    ap.add_argument("--remarks", default=None, help="directory of a MTG_BUILD_REMARKS build: resources per instantiation")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, K, D, B, M = 10, args.segments, 3, args.batch, args.spheres
    box, margin, inflation = 10.0, 1.0, 0.2                     # random_waypoint_batch's box
    wanted = args.sides.split(",")
    rng = np.random.default_rng(2025)
    centres, radii = rng.uniform(-box, box, (M, 3)), rng.uniform(0.5, 1.5, M)
    res = resources(args.remarks) if args.remarks else None
    if res is not None:
        assert len(res) == 20 and all(r["scratch"] == 0 for r in res.values()), res
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
        longest = max(float(t.sum(dim=1).max()) for _, t in bufs)
        n_samples = int(np.ceil(longest / args.dt)) + 1
        span = 2.0 * (box + margin)
        h = span / 255.0
        lo = -(box + margin)
        small = m.DistanceField(spheres_field((256, 256, 256), (lo, lo, lo), h, centres, radii), (lo, lo, lo), h)
        nearest = m.DistanceField(small.distances, small.origin, h, interpolation="nearest")
        fields = {"a": small, "a_nearest": nearest}
        if "a_big" in wanted:
            hb = span / 511.0
            zlo = -0.5 * 319 * hb
            fields["a_big"] = m.DistanceField(spheres_field((512, 512, 320), (lo, lo, zlo), hb, centres, radii), (lo, lo, zlo), hb)
        comparator = Comparator(ctx, small, args.dt, n_samples, inflation)

        def check(i, field, lanes=None):
            if lanes is not None:
                ctx.set_option("field_lanes", lanes)
            r = m.check_distance_field(ctx, *bufs[i % n_buf], field, args.dt, inflation=inflation, max_samples=1 << 16)
            if lanes is not None:
                ctx.set_option("field_lanes", 0)
            return r

        sides = {"a": lambda i: check(i, small), "a_nearest": lambda i: check(i, nearest), "b": lambda i: comparator(*bufs[i % n_buf])}
        for g in (1, 4, 16, 64):
            sides[f"a_lanes{g}"] = lambda i, g=g: check(i, small, g)
        if "a_big" in fields:
            sides["a_big"] = lambda i: check(i, fields["a_big"])
        sides = {k: v for k, v in sides.items() if k in wanted}

        # the default call against the host form on the first trajectories, and the five group sizes against each other
        full = check(0, small)
        ctx.sync()
        nb = min(64, B)
        co, t = bufs[0][0][:nb].cpu().numpy(), bufs[0][1][:nb].cpu().numpy()
        host = m.check_distance_field_host(co, t, m.DistanceField(small.distances.cpu().numpy(), small.origin, h), args.dt, inflation=inflation,
                                           max_samples=1 << 16)
        for name in ("trajectory_feasible", "first_failing_segment", "segment_closest_sample", "segment_first_failing_sample", "segment_samples"):
            assert np.array_equal(getattr(full, name)[:nb].cpu().numpy(), getattr(host, name)), name
        assert np.abs(full.segment_clearance[:nb].cpu().numpy() - host.segment_clearance).max() <= 1e-12
        for g in (1, 4, 16, 64):
            other = check(0, small, g)
            ctx.sync()
            assert all(torch.equal(a, b) for a, b in zip(other[:7], full[:7])), g
        samples = full.segment_samples.double()
        stats = {"samples_per_segment_mean": round(float(samples.mean()), 1), "samples_per_segment_max": int(samples.max()),
                 "feasible_trajectories": int(full.trajectory_feasible.sum()), "comparator_samples_per_trajectory": n_samples}
        if "b" in sides:
            fb, cb = comparator(*bufs[0])
            ctx.sync()
            stats["comparator_feasible_trajectories"] = int(fb.sum())
            stats["outside_share"] = round(comparator.outside_share, 4)

        for name, fn in sides.items():
            timed(ctx, fn, 2 if name == "b" else args.warmup)
        runs = {k: [] for k in sides}
        for _ in range(args.repeats):
            for name, fn in sides.items():
                runs[name].append(timed(ctx, fn, args.calls_b if name == "b" else args.calls))
        plan.close()
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    spread = {k: round(100.0 * (max(v) - min(v)) / med[k], 2) for k, v in runs.items()}
    out = {"tool": "bench_distance_field", "N": N, "K": K, "D": D, "batch": B, "spheres": M, "dt": args.dt, "inflation": inflation,
           "calls": args.calls, "calls_b": args.calls_b, "repeats": args.repeats, "buffers": n_buf,
           "field": [256, 256, 256], "field_mib": 64, "big_field": [512, 512, 320], "big_field_mib": 320, **stats,
           "us": {k: round(v, 1) for k, v in med.items()}, "spread_percent": spread,
           "runs_us": {k: [round(x, 1) for x in v] for k, v in runs.items()}, "resources": res}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
