"""Device time of the batched distance-field collision cost and gradient (A: one collision_cost call with the gradient; A0: the
same call, cost only) against what the library offered before for the same numbers (B): sample_range(n_derivatives=2) with every
segment as a trajectory of its own (local times 0, i dt, and the end beyond T: the call's own sample set), over the longest
segment, then the weights, index arithmetic, eight gathers, interpolation, the field's gradient, the potential, the speed and the
two Vandermonde contractions to [B][K][3][N] as torch operations on the device, a chunk of trajectories at a time.  B computes
the same sums in another order: its trajectory costs must agree with A's within 1e-9 relative (asserted), which shows that it
does the same work.  Required: A < B.  `field`: check_distance_field on the same inputs, for scale.

Protocol of tools/bench_distance_field.py, whose workload this is (10k x 8, N = 10, dt = 0.01, a 256^3 float32 field of 16 spheres in
the waypoint box, inflation 0.2; here with epsilon = 0.5 and speed_epsilon = 1e-3): one process; device events around `--calls`
back-to-back calls after a warm-up; the inputs rotate over enough coefficient buffers that they come from HBM (more than 512 MB of
them); the sides alternate and the round is repeated `--repeats` times, the spread over the repeats is reported with the median.
Next to the times: samples per segment, the share of samples with c > 0, and -- with --remarks <dir of a MTG_BUILD_REMARKS build>
-- VGPRs, AGPRs, scratch and LDS of every instantiation (no scratch: asserted).  Asserted too: the call equals the host form on
the first trajectories.  Prints one JSON line; --out appends it to a file.

    python tools/bench_collision_cost.py [--batch 10000] [--calls 20] [--repeats 5] [--remarks DIR] [--out profiles/collision_cost_bench.jsonl]
"""
import argparse
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
    """{instantiation: {vgprs, agprs, scratch, lds}} of the segment kernels, from the build's resource remarks."""
    text = open(os.path.join(remarks, "mtg_collision.log")).read()
    out = {}
    for name, body in re.findall(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", text, flags=re.S):
        inst = re.search(r"seg_kernelILi(\d+)ELb([01])E", name)
        if not inst:
            continue
        get = lambda key: int(re.search(re.escape(key) + r": (\d+)", body).group(1))
        out[f"N{inst.group(1)}_{'gradient' if inst.group(2) == '1' else 'cost'}"] = {
            "vgprs": get("VGPRs"), "agprs": get("AGPRs"), "scratch": get("ScratchSize [bytes/lane]"), "lds": get("LDS Size [bytes/block]")}
    return out


class Comparator:
    """B: p and v from sample_range, everything after them as tensor operations."""

    def __init__(self, ctx, field, dt, inflation, epsilon, speed_epsilon, chunk):
        self.ctx, self.field, self.dt, self.inflation, self.epsilon, self.eta, self.chunk = ctx, field, dt, inflation, epsilon, speed_epsilon, chunk
        nz, ny, nx = field.distances.shape
        self.flat = field.distances.view(-1)
        self.origin = torch.tensor(field.origin, dtype=torch.float64, device="cuda")
        self.top = torch.tensor([nx - 1, ny - 1, nz - 1], dtype=torch.float64, device="cuda")
        self.stride = (1, nx, nx * ny)
        self.r = 1.0 / field.voxel_size
        self.positive = self.samples = 0
        self.count = False

    def segments(self, coeffs, times):
        """coeffs [Q][1][3][N], times [Q][1]: cost [Q] and gradient [Q][3][N]."""
        q, n = coeffs.shape[0], coeffs.shape[-1]
        T = times[:, 0]
        smax = int(torch.ceil(T.max() / self.dt)) + 2
        i = torch.arange(smax, device="cuda", dtype=torch.float64)
        grid = i * self.dt
        S = (grid[None, 1:] < T[:, None]).sum(dim=1) + 2
        last = (S - 1)[:, None]
        idx = torch.arange(smax, device="cuda")[None, :]
        t = torch.where(idx == last, T[:, None], grid[None, :])                                      # [Q][S]
        valid = idx <= last
        hi = torch.gather(t, 1, torch.minimum(idx + 1, last).expand(q, smax))
        lo = torch.gather(t, 1, (idx - 1).clamp(min=0).expand(q, smax))
        w = torch.where(valid, (hi - lo) * 0.5, torch.zeros_like(t))
        pv = m.sample_range(self.ctx, coeffs, times, 0.0, self.dt, smax, n_derivatives=2)           # [Q][S][2][3]; beyond T: at T
        pos, vel = pv[:, :, 0, :], pv[:, :, 1, :]
        u = (pos - self.origin) * self.r
        inside = ((u >= 0) & (u <= self.top)).all(dim=-1)
        cell = torch.minimum(u.floor().clamp_(min=0.0), self.top - 1)
        f = u - cell
        cell = cell.long()
        base = cell[..., 0] + cell[..., 1] * self.stride[1] + cell[..., 2] * self.stride[2]
        v = [self.flat[base + (dx + dy * self.stride[1] + dz * self.stride[2])].double() for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
        fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
        e00, e10, e01, e11 = (v[j + 1] - v[j] for j in (0, 2, 4, 6))
        x00, x10, x01, x11 = (torch.addcmul(v[j], fx, e) for j, e in zip((0, 2, 4, 6), (e00, e10, e01, e11)))
        y0, y1 = torch.addcmul(x00, fy, x10 - x00), torch.addcmul(x01, fy, x11 - x01)
        d = torch.addcmul(y0, fz, y1 - y0)
        ex0, ex1 = torch.addcmul(e00, fy, e10 - e00), torch.addcmul(e01, fy, e11 - e01)
        G = torch.stack([torch.addcmul(ex0, fz, ex1 - ex0), torch.addcmul(x10 - x00, fz, (x11 - x01) - (x10 - x00)), y1 - y0], dim=-1) * self.r
        d = torch.where(inside, d, torch.full_like(d, self.field.outside_distance))
        G = torch.where(inside[..., None], G, torch.zeros_like(G))
        x = d - self.inflation
        eps = self.epsilon
        c = torch.where(x < 0, 0.5 * eps - x, torch.where(x <= eps, (x - eps) ** 2 / (2 * eps), torch.zeros_like(x)))
        dc = torch.where(x < 0, -torch.ones_like(x), torch.where(x <= eps, (x - eps) / eps, torch.zeros_like(x)))
        s = torch.sqrt((vel * vel).sum(dim=-1) + self.eta * self.eta)
        cost = (w * c * s).sum(dim=1)
        A = (w * dc * s)[..., None] * G                                                               # [Q][S][3]
        Bv = (w * c / s)[..., None] * vel
        j = torch.arange(n, device="cuda", dtype=torch.float64)
        pw = t[..., None] ** j                                                                        # [Q][S][N]
        dpw = j * t[..., None] ** (j - 1).clamp(min=0)
        grad = torch.einsum("qsa,qsj->qaj", A, pw) + torch.einsum("qsa,qsj->qaj", Bv, dpw)
        if self.count:      # (outside the timed calls: reading the counts back waits for the device)
            self.positive += int(((c > 0) & valid).sum())
            self.samples += int(valid.sum())
        return cost, grad

    def __call__(self, coeffs, times):
        b, k, d, n = coeffs.shape
        costs, grads = [], []
        for first in range(0, b, self.chunk):
            co = coeffs[first:first + self.chunk].reshape(-1, 1, d, n)
            cost, grad = self.segments(co, times[first:first + self.chunk].reshape(-1, 1))
            costs.append(cost.view(-1, k))
            grads.append(grad.view(-1, k, 3, n))
        seg = torch.cat(costs)
        return seg.sum(dim=1), seg, torch.cat(grads)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=10_000)
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--spheres", type=int, default=16)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--calls-b", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=1000, help="trajectories per pass of the comparator (bounds its memory)")
    ap.add_argument("--remarks", default=None, help="directory of a MTG_BUILD_REMARKS build: resources per instantiation")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, K, D, B, M = 10, args.segments, 3, args.batch, args.spheres
    box, margin, inflation, epsilon, eta = 10.0, 1.0, 0.2, 0.5, 1e-3
    rng = np.random.default_rng(2025)
    centres, radii = rng.uniform(-box, box, (M, 3)), rng.uniform(0.5, 1.5, M)
    res = resources(args.remarks) if args.remarks else None
    if res is not None:
        assert len(res) == 10 and all(r["scratch"] == 0 for r in res.values()), res
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
        comparator = Comparator(ctx, field, args.dt, inflation, epsilon, eta, args.chunk)
        kw = dict(inflation=inflation, epsilon=epsilon, speed_epsilon=eta, max_samples=1 << 16)
        sides = {"a": lambda i: m.collision_cost(ctx, *bufs[i % n_buf], field, args.dt, **kw),
                 "a0": lambda i: m.collision_cost(ctx, *bufs[i % n_buf], field, args.dt, want_gradient=False, **kw),
                 "field": lambda i: m.check_distance_field(ctx, *bufs[i % n_buf], field, args.dt, inflation=inflation, max_samples=1 << 16),
                 "b": lambda i: comparator(*bufs[i % n_buf])}

        # the call against the host form on the first trajectories, the cost-only call, and the comparator
        full, cost_only = sides["a"](0), sides["a0"](0)
        ctx.sync()
        assert torch.equal(full.segment_cost, cost_only.segment_cost) and torch.equal(full.trajectory_cost, cost_only.trajectory_cost)
        nb = min(32, B)
        co, t = bufs[0][0][:nb].cpu().numpy(), bufs[0][1][:nb].cpu().numpy()
        host = m.collision_cost_host(co, t, m.DistanceField(field.distances.cpu().numpy(), field.origin, h), args.dt, **kw)
        same = all(np.array_equal(getattr(full, name)[:nb].cpu().numpy(), getattr(host, name), equal_nan=True) for name in full._fields)
        scale = np.abs(host.coeff_gradient).max()
        assert np.array_equal(full.segment_samples[:nb].cpu().numpy(), host.segment_samples)
        assert np.abs(full.segment_cost[:nb].cpu().numpy() - host.segment_cost).max() <= 1e-12 * np.abs(host.segment_cost).max()
        assert np.abs(full.coeff_gradient[:nb].cpu().numpy() - host.coeff_gradient).max() <= 1e-12 * scale
        comparator.count = True
        traj_b, seg_b, grad_b = comparator(*bufs[0])
        comparator.count = False
        ctx.sync()
        top = float(traj_b.max())
        big = traj_b > 1e-6 * top
        rel = float(((full.trajectory_cost - traj_b).abs()[big] / traj_b[big]).max())
        small_abs = float((full.trajectory_cost - traj_b).abs()[~big].max()) if bool((~big).any()) else 0.0
        grad_rel = float((full.coeff_gradient - grad_b).abs().max() / grad_b.abs().max())
        assert rel <= 1e-9 and small_abs <= 1e-9 * 1e-6 * top, (rel, small_abs)
        samples = full.segment_samples.double()
        stats = {"samples_per_segment_mean": round(float(samples.mean()), 1), "samples_per_segment_max": int(samples.max()),
                 "share_of_samples_with_positive_cost": round(comparator.positive / comparator.samples, 4),
                 "trajectories_with_positive_cost": int((full.trajectory_cost > 0).sum()),
                 "a_vs_b_trajectory_cost_relative": rel, "a_vs_b_gradient_over_largest": grad_rel, "device_equals_host_bitwise": bool(same)}

        for name, fn in sides.items():
            timed(ctx, fn, 1 if name == "b" else args.warmup)
        runs = {k: [] for k in sides}
        for _ in range(args.repeats):
            for name, fn in sides.items():
                runs[name].append(timed(ctx, fn, args.calls_b if name == "b" else args.calls))
        plan.close()
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    spread = {k: round(100.0 * (max(v) - min(v)) / med[k], 2) for k, v in runs.items()}
    assert med["a"] < med["b"], med
    out = {"tool": "bench_collision_cost", "N": N, "K": K, "D": D, "batch": B, "spheres": M, "dt": args.dt, "inflation": inflation,
           "epsilon": epsilon, "speed_epsilon": eta, "calls": args.calls, "calls_b": args.calls_b, "repeats": args.repeats, "buffers": n_buf,
           "field": [256, 256, 256], "field_mib": 64, **stats, "us": {k: round(v, 1) for k, v in med.items()},
           "b_over_a": round(med["b"] / med["a"], 1), "a_over_field": round(med["a"] / med["field"], 2), "spread_percent": spread,
           "runs_us": {k: [round(x, 1) for x in v] for k, v in runs.items()}, "resources": res}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
