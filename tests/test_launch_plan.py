"""The launch decision (csrc/mtg_launch_plan.h: plan, batch, layout, flags, knobs -> form, kernel, grid, LDS, workspace) as a pure
function, built for the host (tests/launch_plan_emu.cpp) with fabricated table entries whose function pointers are tags.  Every
case is compared field for field, launch for launch, with an independent restatement of the rules written here, at 256 CUs and
at 4; the thresholds named in the case list are additionally asserted as literal outcomes (so a mistake shared by the two
statements of a rule still shows).  Covers what no device test reaches: the 2^31 / 2^32 size limits.  No GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mav_trajectory_generation_amd", "csrc")
GENERIC, FUSED, SPLIT, DIMLANE, ONE_PER_BATCH, COOP = 1 << 1, 1 << 2, 1 << 3, 1 << 5, 1 << 8, 1 << 11      # MTG_FLAG_*
F_GENERIC, F_FUSED, F_SPLIT, F_ROLLED, F_SLAB, F_DIMLANE, F_DIMLANE_RT, F_COOP, F_UPDATE = range(9)          # form codes
KNOBS = dict(force_dg=0, prefer_rolled=0, no_dimlane=0, dl_max_units_per_cu=-1, no_slab=0, no_slab_extra=0, no_dl_extra=0, no_queue=0,
             dl_grid_per_cu=8, dl_rt=-1, no_balance=0, slab_policy=-1, rolled_wg_per_cu=4, coop=-1)
FIELDS = ("fn", "dl", "rt", "coop", "grid", "gridy", "block", "lds", "dim0", "ntiles", "ws_bytes", "ws_stride", "input_kind", "attr", "user_ws")
STATIC_SLOTS = ("fast", "fast_split", "rolled", "g1", "g2", "g3", "g4")
CUS = (256, 4)


def cdiv(a, b):
    return -(-a // b)


def pad16(b):
    return cdiv(b, 16) * 16


# ---- fabricated plans ------------------------------------------------------------------------------------------------------------
def static(d, k, heavy=0, upd=0, upd_slab=0, upd_slab_lds=0):
    return dict(d=d, k=k, heavy=heavy, upd=upd, upd_slab=upd_slab, upd_slab_lds=upd_slab_lds)


def rolled(d, upd_slab_lds=30 * 1024):
    return static(d, -1, upd=1, upd_slab=1, upd_slab_lds=upd_slab_lds)


def dimlane(h, k, np_=2, tpw=21, lo=0, hi=3, lds=60000, ws_per_lane=0, queue=1, extra=1):
    return dict(h=h, k=k, np=np_, tpw=tpw, lo=lo, hi=hi, lds=lds, ws_per_lane=ws_per_lane, queue=queue, extra=extra)


def coop_lds(H, D, K):
    if D != 3 or K < 2 or not 4 <= H <= 6:
        return 0
    f = H - 1
    return (2 * (f + D) * 64 + K * (f + D) * (4 * f + 1)) * 8


def plan(H, D, K, *, interior_fixed=1, coop_shape=True, generic=True, slab=None, dl=None, rt=None, **statics):
    """A plan of the standard family: ends fully fixed, `interior_fixed` derivatives fixed at the K - 1 interior vertices."""
    p = dict(H=H, D=D, K=K, n_fixed=2 * H + (K - 1) * interior_fixed, free_mid=(H - interior_fixed) if K >= 2 else 0,
             coop_shape=coop_shape and interior_fixed == 1, coop_lds=coop_lds(H, D, K), slab=slab, dl=dl, rt=rt, generic=generic)
    for s in STATIC_SLOTS:
        p[s] = statics.pop(s, None)
    assert not statics
    return p


def n10k8():
    """N = 10 / K = 8 / D = 3 as the tables have it: fused + one-dimension static kernels, rolled, slab, dimlane (tpw 21, np 2, lo 0, hi 3)."""
    return plan(5, 3, 8, fast=static(3, 8), fast_split=static(1, 8), rolled=rolled(3), g1=static(1, 8), g3=static(3, 8),
                slab=dict(lds=65024, queue=1, extra=1), dl=dimlane(5, 8), rt=dict(tpw=21, r=13, l=6, lds=50000, step_bytes=4096))


def plain(H=5, D=3, K=8, **kw):
    """The same family without slab and dimension-in-lane entries."""
    kw.setdefault("fast", static(D, K))
    kw.setdefault("fast_split", static(1, K))
    kw.setdefault("rolled", rolled(D))
    return plan(H, D, K, **kw)


def long_chain(H, K, **kw):
    """A long standard chain: rolled fused kernels, the run-time-K body (R, L of the order's table entry); no static variant."""
    r, l = {4: (27, 9), 5: (13, 6), 6: (8, 4)}[H]
    return plan(H, 3, K, fast=rolled(3), fast_split=rolled(1), rolled=rolled(3), g1=rolled(1), g3=rolled(3),
                rt=dict(tpw=21, r=r, l=l, lds=50000, step_bytes=(H * (H - 1) // 2 + 3 * (H - 1)) * 8), **kw)


def layouts(p, B):
    nf, D, K = p["n_fixed"], p["D"], p["K"]
    bs = pad16(B)
    return dict(soa=(1, B, 1, nf * B, B, 1, 1, 1), aos=(K, 1, D * nf, nf, 1, 1, 1, 1), soa16=(1, bs, 1, nf * bs, bs, 1, 1, 1),
                strided=(K + 1, 1, D * nf + 3, nf, 1, 1, 1, 1), negative=(-K, 1, D * nf, nf, 1, 1, 1, 1))


def call(p, B, layout="soa", flags=0, update=0, extra=0, cost_only=0, pert=0):
    cost_only = int(bool(cost_only or pert))          # a perturbed-time launch is a cost-only launch; the cost is an extra output
    return dict(batch=B, L=layouts(p, B)[layout], flags=flags, update=update, extra=int(bool(extra or cost_only)), cost_only=cost_only, pert=pert)


# ---- the rules, restated ---------------------------------------------------------------------------------------------------------
def input_kind(p, L, B):
    nf, D, K = p["n_fixed"], p["D"], p["K"]
    ts_b, ts_k, fs_b, fs_d, fs_c = L[:5]
    for kind, rows in ((0, B), (2, pad16(B))):
        if (ts_b, ts_k, fs_b, fs_d, fs_c) == (1, rows, 1, nf * rows, rows) and (kind == 0 or rows != B):
            return kind
    return 1 if (ts_b, ts_k, fs_b, fs_d, fs_c) == (K, 1, D * nf, nf, 1) else -1


def offsets_fit(p, B, padded):
    return (pad16(B) if padded else B) * 8 * max(p["K"], p["n_fixed"] * p["D"]) < 2 ** 32


def balanced(kn, ntiles, cap):
    if ntiles <= cap or kn["no_balance"]:
        return min(ntiles, cap)
    return cdiv(ntiles, cdiv(ntiles, cap))


def stage_lds(dims, N):
    return 64 * ((dims * N // 2) | 1) * 16


def solve_lds(dims, N, fm):
    return 2 * stage_lds(dims, N) + 2 * (fm * (fm + 1) // 2 + dims * fm) * 64 * 8


def dl_in_default_range(dl, kn, cus, trajectories):
    units = cdiv(cdiv(trajectories, dl["tpw"]), dl["np"])
    hi = 2 * kn["dl_max_units_per_cu"] if kn["dl_max_units_per_cu"] >= 0 else dl["hi"]
    return units >= dl["lo"] * cus and (hi == 0 or 2 * units <= hi * cus)


def launch(**kw):
    base = dict(fn=0, dl=0, rt=0, coop=0, grid=0, gridy=1, block=128, lds=0, dim0=0, ntiles=0, ws_bytes=0, ws_stride=0, input_kind=-1, attr=-1, user_ws=0)
    assert set(kw) <= set(base)
    base.update(kw)
    return base


def dl_launch(dl, cus, per_cu, ntiles, kind, fn):
    units = cdiv(ntiles, dl["np"])
    grid, ws = min(units, cus * per_cu), 0
    if dl["ws_per_lane"]:
        grid = min(units, cus * 4 // (2 * dl["np"]))
        ws = dl["ws_per_lane"] * grid * dl["np"] * 128
    return launch(fn=fn, dl=1, grid=grid, ntiles=ntiles, ws_bytes=ws, input_kind=kind)     # (block and LDS: the entry's own launch function's)


def static_tag(slot, i):
    return 100 * (STATIC_SLOTS.index(slot) + 1) + i


def expected(p, kn, cus, c):
    """(form, launches, error) of a call."""
    H, D, K, N, B, L, flags = p["H"], p["D"], p["K"], 2 * p["H"], c["batch"], c["L"], c["flags"]
    extra, cost_only, pert = c["extra"], c["cost_only"], c["pert"]
    ntiles = cdiv(B, 64) * (K + 1 if pert else 1)
    groups_of_four = [min(4, D - d0) for d0 in range(0, D, 4)]
    kind = input_kind(p, L, B)
    other_family = flags & (GENERIC | FUSED | SPLIT)
    kc = (K + 1) // 2
    if c["update"]:
        uv = None if flags & GENERIC else p["rolled"]
        if uv:
            phase = 1 if (K * D * N * 8) % 64 else 0
            if not kn["no_slab"] and uv["upd_slab"] and uv["upd_slab_lds"] <= 65536:
                fn, lds = static_tag("rolled", 20 + 2 * extra + phase), uv["upd_slab_lds"]
            else:
                fn, lds = static_tag("rolled", 10 + extra), stage_lds(D, N)
            return F_UPDATE, [launch(fn=fn, grid=min(ntiles, 16 * cus), block=64, lds=lds, ntiles=ntiles)], not uv["upd"]
        return F_UPDATE, [launch(fn=2100 + 10 * dc + extra if p["generic"] else 0, grid=min(ntiles, 16 * cus), block=64, lds=stage_lds(dc, N), ntiles=ntiles,
                                 dim0=4 * i) for i, dc in enumerate(groups_of_four)], not p["generic"]
    # row-cooperative
    ts_b, ts_k, fs_b, fs_d, fs_c = L[:5]
    coop_ok = (D == 3 and 4 <= H <= 6 and K >= 2 and not (cost_only or extra or pert) and p["coop_shape"] and 0 < p["coop_lds"] <= 160 * 1024
               and min(L[:5]) >= 0 and ((B - 1) * ts_b + (K - 1) * ts_k) * 8 < 2 ** 32
               and ((B - 1) * fs_b + (D - 1) * fs_d + (p["n_fixed"] - 1) * fs_c) * 8 < 2 ** 32 and B * K * D * N * 8 < 2 ** 32)
    if coop_ok and not other_family and not flags & DIMLANE:
        take = bool(flags & COOP) or kn["coop"] == 1
        if not take and kn["coop"] != 0 and kn["dl_rt"] != 1 and K >= {6: 16, 5: 64, 4: 80}[H]:
            per_cu = min(2 if (H == 6 and K >= 32) else 1, 160 * 1024 // p["coop_lds"])
            take = cdiv(B, 4) <= per_cu * cus
        if take:
            return F_COOP, [launch(coop=1)], False                     # (grid and LDS: mtg_coop_launch derives them from the batch)
    # run-time-K dimension-in-lane
    rt, dl = p["rt"], p["dl"]
    if (rt and kn["dl_rt"] != 0 and not kn["no_dimlane"] and not (cost_only or extra) and (not dl or kn["dl_rt"] == 1) and not other_family
            and kind in (0, 1) and B + rt["tpw"] < 2 ** 31):
        nt = cdiv(B, rt["tpw"])
        grid = min(nt, 2 * cus)
        ws = rt["step_bytes"] * (kc - 1 - rt["r"]) * grid * 128 if kc - 1 - rt["r"] - rt["l"] > 0 else 0
        return F_DIMLANE_RT, [launch(fn=3100, rt=1, grid=grid, ntiles=nt, ws_bytes=ws, input_kind=kind)], False
    # static dimension-in-lane
    if dl and not kn["no_dimlane"] and not cost_only and not other_family and kind >= 0 and offsets_fit(p, B, True):
        ok = not extra or (dl["extra"] and not kn["no_dl_extra"] and not (dl["h"] == 6 and dl["k"] == 32 and B > 20000 and not flags & DIMLANE))
        if ok and (flags & DIMLANE or dl_in_default_range(dl, kn, cus, B)):
            return F_DIMLANE, [dl_launch(dl, cus, kn["dl_grid_per_cu"], cdiv(B, dl["tpw"]), kind, 3000)], False
    # fused family: which static entry
    def slab_for(slot):
        e = p[slot] if slot else None
        return p["slab"] if e and e["k"] > 0 and e["d"] == D and not kn["no_slab"] else None
    coeffs_only = not (extra or cost_only or pert)
    if flags & GENERIC:
        var = None
    elif coeffs_only and not flags & SPLIT and kn["force_dg"] <= 0 and not kn["prefer_rolled"] and slab_for("fast"):
        var = "fast"
    else:
        auto_split = ntiles < 4 * cus
        if p["fast"] and p["fast_split"] and not p["fast"]["heavy"]:
            auto_split = ntiles * (D // p["fast_split"]["d"]) <= 4 * cus
        want_split = bool(flags & SPLIT) or (not flags & FUSED and auto_split)
        var = "fast_split" if want_split and p["fast_split"] else ("fast" if p["fast"] else ("fast_split" if p["fast_split"] else None))
        if var and p[var]["heavy"] and not want_split and p["rolled"]:
            var = "rolled"
        if kn["prefer_rolled"] and p["rolled"]:
            var = "rolled"
        dg = kn["force_dg"]
        if 1 <= dg <= 4 and D % dg == 0 and p["g%d" % dg]:
            var = "g%d" % dg
    slab = None if cost_only or pert else slab_for(var)
    if slab and extra and (not slab["extra"] or kn["no_slab_extra"]):
        slab = None
    if slab:
        pol = kn["slab_policy"] if kn["slab_policy"] >= 0 else 1
        return F_SLAB, [launch(fn=1003 if extra else 1000 + pol, grid=balanced(kn, ntiles, 2 * cus), lds=slab["lds"], ntiles=ntiles,
                               attr=2 if extra else pol)], False
    fm = p["free_mid"]
    if var:
        e = p[var]
        ngroups = D // e["d"]
        wt = ntiles * ngroups <= 4 * cus
        fn = static_tag(var, 4 if cost_only else extra + 2 * wt)
        l = launch(fn=fn, grid=min(ntiles, max(1, 8 * cus // ngroups)), gridy=ngroups, lds=solve_lds(e["d"], N, fm), ntiles=ntiles, user_ws=1)
        if e["k"] < 0:
            l["grid"] = min(ntiles, max(1, cus * kn["rolled_wg_per_cu"] // ngroups))
            l["ws_stride"] = l["grid"] * ngroups * 128
            l["ws_bytes"] = kc * (H * H + e["d"] * H) * l["ws_stride"] * 8
        return (F_ROLLED if e["k"] < 0 else F_FUSED if e["d"] == D else F_SPLIT), [l], False
    out = []
    for i, dc in enumerate(groups_of_four):
        grid = min(ntiles, 4 * cus)
        out.append(launch(fn=(2000 + 10 * dc + (2 if cost_only else extra)) if p["generic"] else 0, grid=grid, lds=solve_lds(dc, N, fm), ntiles=ntiles, dim0=4 * i,
                          ws_stride=grid * 128, ws_bytes=kc * (H * H + dc * H) * grid * 128 * 8))
    return F_GENERIC, out, not p["generic"]


def expected_queue(p, kn, cus, n, B, L, flags):
    """(slab chosen, dimlane chosen, tiles per batch, launches) of a queue of n batches."""
    if n < 2 or B <= 0 or kn["no_queue"] or flags & (GENERIC | SPLIT | ONE_PER_BATCH):
        return 0, 0, None, []
    per_launch = min(n, 96)
    kind = input_kind(p, L, B)
    f = p["fast"]
    slab = p["slab"] if (not flags & DIMLANE and not kn["no_slab"] and f and f["k"] > 0 and f["d"] == p["D"]) else None
    if slab and (not slab["queue"] or cdiv(B, 64) * per_launch >= 2 ** 31):
        slab = None
    dl = p["dl"]
    if dl and (not dl["queue"] or kn["no_dimlane"] or flags & FUSED or kind < 0 or not offsets_fit(p, B, True) or cdiv(B, dl["tpw"]) * per_launch >= 2 ** 31):
        dl = None
    if slab and dl and not flags & DIMLANE and not dl_in_default_range(dl, kn, cus, B * per_launch):
        dl = None
    if not slab and not dl:
        return 0, 0, None, []
    tpb = cdiv(B, dl["tpw"] if dl else 64)
    out = []
    for i0 in range(0, n, 96):
        nt = min(96, n - i0) * tpb
        out.append(dl_launch(dl, cus, 8, nt, kind, 3001) if dl else launch(fn=1002, grid=balanced(kn, nt, 2 * cus), lds=slab["lds"], ntiles=nt, attr=3))
    return int(bool(slab)), int(bool(dl)), tpb, out


# ---- the library's answers -------------------------------------------------------------------------------------------------------
def plan_ints(p):
    v = [p["H"], p["D"], p["K"], p["n_fixed"], p["free_mid"], int(p["coop_shape"]), p["coop_lds"]]
    for s in STATIC_SLOTS:
        e = p[s]
        v += [1, e["d"], e["k"], e["heavy"], e["upd"], e["upd_slab"], e["upd_slab_lds"]] if e else [0] * 7
    s, d, r = p["slab"], p["dl"], p["rt"]
    v += [1, s["lds"], s["queue"], s["extra"]] if s else [0] * 4
    v += [1, d["h"], d["k"], d["np"], d["tpw"], d["lo"], d["hi"], d["lds"], d["ws_per_lane"], d["queue"], d["extra"]] if d else [0] * 11
    v += [1, r["tpw"], r["r"], r["l"], r["lds"], r["step_bytes"]] if r else [0] * 6
    return v + [int(p["generic"])]


def knob_ints(kn):
    return [kn[k] for k in KNOBS]


def call_ints(c):
    return [c["batch"], *c["L"], c["flags"], c["update"], c["extra"], c["cost_only"], c["pert"]]


def arr(v):
    return np.ascontiguousarray(v, dtype=np.int64)


def load_emu():
    so, src = os.path.join(ROOT, "tests", "libmtg_launch_plan_emu.so"), os.path.join(ROOT, "tests", "launch_plan_emu.cpp")
    deps = [src, os.path.join(ROOT, "include", "mtg_hip.h"), os.path.join(CSRC, "mtg_launch_plan.h"), os.path.join(CSRC, "mtg_entries.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    lp = ctypes.POINTER(ctypes.c_longlong)
    for fn in (lib.mtg_launch_plan_emu, lib.mtg_queue_plan_emu):
        fn.argtypes = [lp, lp, ctypes.c_int, lp, ctypes.c_int, lp]
    lib.mtg_launch_rule_emu.argtypes = [lp, lp, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong]
    lib.mtg_launch_rule_emu.restype = ctypes.c_longlong
    return lib


@pytest.fixture(scope="module")
def emu():
    return load_emu()


def ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))


def decide(lib, p, kn, cus, c):
    out = np.full(3 + 15 * 8, -99, dtype=np.int64)
    n = lib.mtg_launch_plan_emu(ptr(arr(plan_ints(p))), ptr(arr(knob_ints(kn))), cus, ptr(arr(call_ints(c))), 8, ptr(out))
    assert n == out[1] and 1 <= n <= 8
    return int(out[0]), [dict(zip(FIELDS, out[3 + 15 * i:18 + 15 * i].tolist())) for i in range(n)], bool(out[2])


def decide_queue(lib, p, kn, cus, n, B, L, flags):
    out = np.full(5 + 15 * 8, -99, dtype=np.int64)
    q = arr([n, B, *L, flags])
    m = lib.mtg_queue_plan_emu(ptr(arr(plan_ints(p))), ptr(arr(knob_ints(kn))), cus, ptr(q), 8, ptr(out))
    assert m == out[4] and m <= 8
    return int(out[0]), int(out[1]), int(out[2]) if m else None, [dict(zip(FIELDS, out[5 + 15 * i:20 + 15 * i].tolist())) for i in range(m)]


def check(lib, p, c, cus=CUS, **knobs):
    """The library's decision == the restatement at every CU count; returns the forms (one per CU count) and the launches at cus[0]."""
    kn = dict(KNOBS, **knobs)
    forms, first = [], None
    for n_cu in cus:
        got, want = decide(lib, p, kn, n_cu, c), expected(p, kn, n_cu, c)
        assert got[0] == want[0] and got[2] == want[2], (n_cu, c, got, want)
        assert len(got[1]) == len(want[1])
        for i, (g, w) in enumerate(zip(got[1], want[1])):
            assert g == w, (n_cu, c, i, {k: (g[k], w[k]) for k in FIELDS if g[k] != w[k]})
        forms.append(got[0])
        first = first or got[1]
    return forms, first


def rule(lib, p, which, a, b, c=0, cus=256, **knobs):
    """One of the small shared rules (see mtg_launch_rule_emu)."""
    return lib.mtg_launch_rule_emu(ptr(arr(plan_ints(p))), ptr(arr(knob_ints(dict(KNOBS, **knobs)))), cus, which, a, b, c)


def form(lib, p, c, cus=256, **knobs):
    """The form at `cus` CUs, for a literal assertion; the decision is held to the restatement at every count of CUS as well."""
    counts = CUS if cus in CUS else CUS + (cus,)
    return check(lib, p, c, cus=counts, **knobs)[0][counts.index(cus)]


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def test_dimlane_to_slab_edge(emu):
    """N = 10 / K = 8 / D = 3 (tpw 21, np 2, hi 3): 1.5 workgroups per CU = 384 units of 42 trajectories = 16128."""
    p = n10k8()
    for layout in ("soa", "aos", "soa16"):
        assert check(emu, p, call(p, 16128, layout))[0] == [F_DIMLANE, F_SLAB]      # (4 CUs: 6 units)
        assert check(emu, p, call(p, 16129, layout))[0][0] == F_SLAB
    assert check(emu, p, call(p, 6 * 42))[0][1] == F_DIMLANE and check(emu, p, call(p, 6 * 42 + 1))[0][1] == F_SLAB
    assert form(emu, p, call(p, 16129, flags=DIMLANE)) == F_DIMLANE
    assert form(emu, p, call(p, 16129, flags=SPLIT)) == F_SPLIT
    assert form(emu, p, call(p, 16129, flags=FUSED)) == F_SLAB
    assert form(emu, p, call(p, 16129, "strided", flags=DIMLANE)) == F_SLAB          # not a layout the form reads
    assert form(emu, p, call(p, 100, "strided")) == F_SLAB
    assert form(emu, p, call(p, 16129), dl_max_units_per_cu=2) == F_DIMLANE           # 2 x 256 units = 21504
    assert form(emu, p, call(p, 21504), dl_max_units_per_cu=2) == F_DIMLANE and form(emu, p, call(p, 21505), dl_max_units_per_cu=2) == F_SLAB
    assert form(emu, p, call(p, 16128), dl_max_units_per_cu=1) == F_SLAB and form(emu, p, call(p, 10 ** 6), dl_max_units_per_cu=0) == F_DIMLANE
    assert form(emu, p, call(p, 100), no_dimlane=1) == F_SLAB and form(emu, p, call(p, 100), no_dimlane=1, no_slab=1) == F_SPLIT
    lo = dict(p, dl=dimlane(5, 8, lo=1))                                                # a lower limit: 256 units
    assert form(emu, lo, call(lo, 255 * 42)) == F_SLAB and form(emu, lo, call(lo, 255 * 42 + 1)) == F_DIMLANE


def test_split_fused_rule(emu):
    """ntiles x D / d_split <= 4 x CUs on a plan without slab and dimension-in-lane entries: 341 tiles x 3 <= 1024 < 342 x 3."""
    p = plain()
    assert check(emu, p, call(p, 341 * 64))[0][0] == F_SPLIT and check(emu, p, call(p, 341 * 64 + 1))[0][0] == F_FUSED
    assert form(emu, p, call(p, 5 * 64), cus=4) == F_SPLIT and form(emu, p, call(p, 5 * 64 + 1), cus=4) == F_FUSED
    assert form(emu, p, call(p, 64, flags=FUSED)) == F_FUSED and form(emu, p, call(p, 10 ** 6, flags=SPLIT)) == F_SPLIT
    assert form(emu, p, call(p, 64, flags=GENERIC)) == F_GENERIC
    # a heavy fused kernel: the plain tile count (ntiles < 4 x CUs) decides, and above it the rolled form runs
    heavy = plan(5, 4, 16, interior_fixed=3, fast=static(4, 16, heavy=1), fast_split=static(1, 16), rolled=rolled(4), g1=static(1, 16), g2=static(2, 16),
                 g4=static(4, 16, heavy=1))
    assert form(emu, heavy, call(heavy, 1023 * 64)) == F_SPLIT and form(emu, heavy, call(heavy, 1023 * 64 + 1)) == F_ROLLED
    assert form(emu, heavy, call(heavy, 64, flags=FUSED)) == F_ROLLED
    assert form(emu, dict(heavy, rolled=None), call(heavy, 64, flags=FUSED)) == F_FUSED
    # knobs
    assert form(emu, p, call(p, 64), prefer_rolled=1) == F_ROLLED and form(emu, dict(p, rolled=None), call(p, 64), prefer_rolled=1) == F_SPLIT
    assert form(emu, heavy, call(heavy, 10 ** 6), force_dg=2) == F_SPLIT            # 2 divides 4
    assert check(emu, heavy, call(heavy, 10 ** 6), force_dg=2)[1][0]["gridy"] == 2
    assert form(emu, heavy, call(heavy, 10 ** 6), force_dg=3) == F_ROLLED           # 3 does not: ignored
    assert form(emu, heavy, call(heavy, 10 ** 6), force_dg=8) == F_ROLLED
    pg = plain(g1=static(1, 8), g3=static(3, 8))
    assert form(emu, pg, call(pg, 64), force_dg=3) == F_FUSED and form(emu, pg, call(pg, 10 ** 6), force_dg=1) == F_SPLIT
    assert form(emu, p, call(p, 64), force_dg=3) == F_SPLIT                         # no entry of that group size: ignored
    q = n10k8()
    assert form(emu, q, call(q, 10 ** 6), force_dg=3) == F_SLAB and form(emu, q, call(q, 10 ** 6), force_dg=1) == F_SPLIT
    assert form(emu, q, call(q, 10 ** 6), prefer_rolled=1) == F_ROLLED
    # only a split entry / no entry at all
    only_split = plan(5, 3, 8, fast_split=static(1, 8), g1=static(1, 8))
    assert form(emu, only_split, call(only_split, 10 ** 6)) == F_SPLIT
    none = plan(5, 3, 8, interior_fixed=2)
    assert form(emu, none, call(none, 1000)) == F_GENERIC


def test_write_through(emu):
    """Write-through stores while ntiles x groups <= 4 x CUs: kernel index + 2."""
    p = plain()
    fused = lambda B: check(emu, p, call(p, B, flags=FUSED))[1][0]["fn"]
    assert fused(1024 * 64) == static_tag("fast", 2) and fused(1024 * 64 + 1) == static_tag("fast", 0)
    split = lambda B, **kw: check(emu, p, call(p, B, flags=SPLIT, **kw))[1][0]["fn"]
    assert split(341 * 64) == static_tag("fast_split", 2) and split(341 * 64 + 1) == static_tag("fast_split", 0)
    assert split(341 * 64, extra=1) == static_tag("fast_split", 3) and split(342 * 64, extra=1) == static_tag("fast_split", 1)
    assert split(64, cost_only=1) == static_tag("fast_split", 4)
    assert check(emu, p, call(p, 16 * 64, flags=FUSED), cus=(4,))[1][0]["fn"] == static_tag("fast", 2)
    assert check(emu, p, call(p, 16 * 64 + 1, flags=FUSED), cus=(4,))[1][0]["fn"] == static_tag("fast", 0)


def test_extra_outputs(emu):
    p = n10k8()
    assert form(emu, p, call(p, 1000, extra=1)) == F_DIMLANE and form(emu, p, call(p, 1000, extra=1), no_dl_extra=1) == F_SPLIT
    assert form(emu, p, call(p, 1000, extra=1, flags=DIMLANE), no_dl_extra=1) == F_SPLIT
    assert check(emu, p, call(p, 10 ** 5, extra=1))[1][0]["fn"] == 1003 and check(emu, p, call(p, 10 ** 5, extra=1))[1][0]["attr"] == 2
    no_dl_extra = dict(p, dl=dimlane(5, 8, extra=0))
    assert form(emu, no_dl_extra, call(p, 1000, extra=1)) == F_SPLIT and form(emu, no_dl_extra, call(p, 1000)) == F_DIMLANE
    assert form(emu, p, call(p, 10 ** 5, extra=1)) == F_SLAB and form(emu, p, call(p, 10 ** 5, extra=1), no_slab_extra=1) == F_FUSED
    assert form(emu, dict(p, slab=dict(lds=65024, queue=1, extra=0)), call(p, 10 ** 5, extra=1)) == F_FUSED
    assert form(emu, p, call(p, 100, extra=1), no_dimlane=1, no_slab_extra=1) == F_SPLIT       # with extra outputs the slab does not hold the split form off
    # cost-only and perturbed-time launches: never the slab, the dimension-in-lane or the cooperative form
    assert form(emu, p, call(p, 10 ** 5, cost_only=1)) == F_FUSED and form(emu, p, call(p, 10 ** 5, pert=1)) == F_FUSED
    assert form(emu, p, call(p, 100, cost_only=1)) == F_SPLIT and form(emu, p, call(p, 100, pert=1, flags=DIMLANE)) == F_SPLIT
    assert check(emu, p, call(p, 1000, pert=1))[1][0]["ntiles"] == 16 * 9
    # N = 12 / K = 32 with extra outputs: dimension-in-lane up to 20000 trajectories, unless forced
    k32 = plan(6, 3, 32, fast=rolled(3), fast_split=rolled(1), rolled=rolled(3), g1=rolled(1), g3=rolled(3), dl=dimlane(6, 32, np_=1, hi=0, ws_per_lane=7 * 80))
    assert form(emu, k32, call(k32, 20000, extra=1), coop=0) == F_DIMLANE and form(emu, k32, call(k32, 20001, extra=1), coop=0) == F_ROLLED
    assert form(emu, k32, call(k32, 20001, extra=1, flags=DIMLANE)) == F_DIMLANE and form(emu, k32, call(k32, 20001), coop=0) == F_DIMLANE
    k16 = dict(k32, dl=dimlane(6, 16, np_=1, hi=0))
    assert form(emu, k16, call(k16, 20001, extra=1), coop=0) == F_DIMLANE


def test_row_cooperative(emu):
    for H, kmin in ((6, 16), (5, 64), (4, 80)):
        for K, want in ((kmin - 1, F_DIMLANE_RT), (kmin, F_COOP)):
            p = long_chain(H, K)
            assert form(emu, p, call(p, 8)) == want, (H, K)
    p16, p32 = long_chain(6, 16), long_chain(6, 32)
    assert check(emu, p16, call(p16, 1024))[0] == [F_COOP, F_DIMLANE_RT] and form(emu, p16, call(p16, 1025)) == F_DIMLANE_RT     # one workgroup per CU
    assert form(emu, p16, call(p16, 16), cus=4) == F_COOP and form(emu, p16, call(p16, 17), cus=4) == F_DIMLANE_RT
    assert form(emu, p32, call(p32, 2048)) == F_COOP and form(emu, p32, call(p32, 2049)) == F_DIMLANE_RT                           # K >= 32: two
    # the LDS residency cap: K = 100 at N = 12 needs 135 680 bytes -- eligible, one workgroup per CU although K >= 32; K = 121 no longer fits
    p100, p121 = long_chain(6, 100), long_chain(6, 121)
    assert 81920 < p100["coop_lds"] <= 160 * 1024 < p121["coop_lds"]
    assert form(emu, p100, call(p100, 1024)) == F_COOP and form(emu, p100, call(p100, 1025)) == F_DIMLANE_RT
    assert form(emu, p121, call(p121, 8, flags=COOP)) == F_DIMLANE_RT
    # excluded by flags, outputs, shapes, strides; forced by flag and option
    for fl, want in ((GENERIC, F_GENERIC), (FUSED, F_ROLLED), (SPLIT, F_ROLLED), (DIMLANE, F_DIMLANE_RT)):
        assert form(emu, p16, call(p16, 8, flags=fl)) == want and form(emu, p16, call(p16, 8, flags=fl | COOP)) == want
    assert form(emu, p16, call(p16, 8, extra=1)) == F_ROLLED and form(emu, p16, call(p16, 8, cost_only=1)) == F_ROLLED
    assert form(emu, p16, call(p16, 8, pert=1)) == F_ROLLED
    assert form(emu, dict(p16, coop_shape=False), call(p16, 8, flags=COOP)) == F_DIMLANE_RT
    assert form(emu, p16, call(p16, 8, "negative", flags=COOP)) == F_ROLLED
    assert form(emu, p16, call(p16, 8, "strided")) == F_COOP                                                                      # any non-negative strides
    d4 = plan(6, 4, 16, fast=rolled(4), rolled=rolled(4))
    assert form(emu, d4, call(d4, 8, flags=COOP)) == F_ROLLED
    small = long_chain(6, 8)
    assert form(emu, small, call(small, 8)) == F_DIMLANE_RT and form(emu, small, call(small, 8, flags=COOP)) == F_COOP
    assert form(emu, small, call(small, 10 ** 5), coop=1) == F_COOP and form(emu, p16, call(p16, 8), coop=0) == F_DIMLANE_RT
    assert form(emu, p16, call(p16, 8, flags=COOP), coop=0) == F_COOP
    assert form(emu, p16, call(p16, 8), dl_rt=1) == F_DIMLANE_RT and form(emu, p16, call(p16, 8, flags=COOP), dl_rt=1) == F_COOP
    # the 32-bit limits: coefficient bytes B K D N 8, input offsets
    edge = 2 ** 32 // (16 * 3 * 12 * 8)                     # the last batch with B K D N 8 < 2^32
    assert edge * 4608 < 2 ** 32 <= (edge + 1) * 4608
    assert form(emu, p16, call(p16, edge, flags=COOP)) == F_COOP and form(emu, p16, call(p16, edge + 1, flags=COOP)) == F_DIMLANE_RT
    wide = dict(call(p16, 1000, flags=COOP))
    nf = p16["n_fixed"]
    fs_edge, ts_edge = (2 ** 29 - 1 - (3 * nf - 1)) // 999, (2 ** 29 - 1 - 15) // 999      # the last strides whose largest offset x 8 < 2^32
    for fs_b, want in ((fs_edge, F_COOP), (fs_edge + 1, F_ROLLED)):
        wide["L"] = (16, 1, fs_b, nf, 1, 1, 1, 1)
        assert (((999 * fs_b + 2 * nf + nf - 1) * 8) < 2 ** 32) == (want == F_COOP)
        assert form(emu, p16, wide) == want
    for ts_b, want in ((ts_edge, F_COOP), (ts_edge + 1, F_ROLLED)):
        wide["L"] = (ts_b, 1, 3 * nf, nf, 1, 1, 1, 1)
        assert (((999 * ts_b + 15) * 8) < 2 ** 32) == (want == F_COOP)
        assert form(emu, p16, wide) == want


def test_dimlane_rt(emu):
    p50, p34 = long_chain(5, 50), long_chain(5, 34)
    forms, (l,) = check(emu, p50, call(p50, 10 ** 5))
    assert forms == [F_DIMLANE_RT] * 2 and l["grid"] == 512 and l["ntiles"] == 4762           # min(nt, 2 x CUs)
    assert l["ws_bytes"] == p50["rt"]["step_bytes"] * 11 * 512 * 128                             # 25 - 1 - 13 head-step slots (6 of them LDS steps)
    assert check(emu, p50, call(p50, 100))[1][0]["grid"] == 5
    assert check(emu, p34, call(p34, 10 ** 5))[1][0]["ws_bytes"] == 0                            # 17 - 1 - 13 - 6 < 0: no head step
    p42, p40 = long_chain(5, 42), long_chain(5, 40)
    assert check(emu, p42, call(p42, 64))[1][0]["ws_bytes"] == p42["rt"]["step_bytes"] * 7 * 4 * 128 and check(emu, p40, call(p40, 64))[1][0]["ws_bytes"] == 0
    assert form(emu, p50, call(p50, 1000, "aos")) == F_DIMLANE_RT
    assert form(emu, p50, call(p50, 1001, "soa16")) == F_ROLLED                                  # padded SoA: the static variants only
    assert form(emu, p50, call(p50, 1000, "strided")) == F_ROLLED
    assert form(emu, p50, call(p50, 1000), dl_rt=0) == F_ROLLED and form(emu, p50, call(p50, 1000), no_dimlane=1) == F_ROLLED
    assert form(emu, p50, call(p50, 1000, extra=1)) == F_ROLLED and form(emu, p50, call(p50, 1000, flags=FUSED)) == F_ROLLED
    p = n10k8()                                                                                  # a static variant exists: only with dl_rt = 1
    assert form(emu, p, call(p, 1000)) == F_DIMLANE and form(emu, p, call(p, 1000), dl_rt=1) == F_DIMLANE_RT
    assert form(emu, p, call(p, 1001, "soa16"), dl_rt=1) == F_DIMLANE
    # B + tpw >= 2^31: refused (SoA strides of such a batch are only numbers here)
    assert form(emu, p50, call(p50, 2 ** 31 - 22)) == F_DIMLANE_RT and form(emu, p50, call(p50, 2 ** 31 - 21)) == F_ROLLED


def test_grids(emu):
    p = n10k8()
    assert rule(emu, p, 4, 3140, 512) == 449 and rule(emu, p, 4, 3140, 512, no_balance=1) == 512 and rule(emu, p, 4, 512, 512) == 512
    assert rule(emu, p, 4, 513, 512) == 257 and rule(emu, p, 4, 7, 512) == 7
    # just below 2^31 tiles (a queue's limit): ntiles + cap - 1 no longer fits 32 bits; the rounds are counted in 64
    for nt in (2 ** 31 - 1, 2 ** 31 - 32, 2 ** 31 - 512, 2 ** 31 - 513):
        assert rule(emu, p, 4, nt, 512) == balanced(KNOBS, nt, 512) == cdiv(nt, cdiv(nt, 512)) and rule(emu, p, 4, nt, 512, no_balance=1) == 512
    assert rule(emu, p, 4, 2 ** 31 - 1, 512) == 512 and rule(emu, p, 4, 2 ** 31 - 513, 512) == 512 and rule(emu, p, 4, 2 ** 31 - 1, 3 * 2 ** 29) == 1073741824
    assert check(emu, p, call(p, 3140 * 64))[1][0]["grid"] == 449 and check(emu, p, call(p, 3140 * 64), no_balance=1)[1][0]["grid"] == 512
    assert check(emu, p, call(p, 3140 * 64), slab_policy=0)[1][0]["fn"] == 1000 and check(emu, p, call(p, 3140 * 64))[1][0]["attr"] == 1
    # dimension-in-lane grids: 8 workgroups per CU (option), long chains CUs x 4 / (2 np) with their workspace
    big = dict(p, dl=dimlane(5, 8, hi=0))
    assert check(emu, big, call(big, 10 ** 6))[1][0]["grid"] == 2048 and check(emu, big, call(big, 10 ** 6), dl_grid_per_cu=3)[1][0]["grid"] == 768
    for np_, grid in ((1, 512), (2, 256)):
        ws = dict(p, dl=dimlane(6, 32, np_=np_, hi=0, ws_per_lane=560))
        l = check(emu, ws, call(ws, 10 ** 6), dl_grid_per_cu=3)[1][0]
        assert l["grid"] == grid and l["ws_bytes"] == 560 * grid * np_ * 128
    assert check(emu, ws, call(ws, 100))[1][0]["grid"] == 3
    # rolled grid: rolled_wg_per_cu workgroups per CU over the dimension groups; its workspace
    r = long_chain(5, 50)
    l = check(emu, r, call(r, 10 ** 6, flags=FUSED))[1][0]
    assert l["grid"] == 1024 and l["ws_stride"] == 1024 * 128 and l["ws_bytes"] == 25 * (25 + 15) * 1024 * 128 * 8 and l["user_ws"] == 1
    assert check(emu, r, call(r, 10 ** 6, flags=FUSED), rolled_wg_per_cu=2)[1][0]["grid"] == 512
    l = check(emu, r, call(r, 10 ** 6, flags=SPLIT), rolled_wg_per_cu=2)[1][0]
    assert (l["grid"], l["gridy"], l["ws_stride"]) == (170, 3, 170 * 3 * 128)
    assert check(emu, r, call(r, 10 ** 6, flags=SPLIT), cus=(1,), rolled_wg_per_cu=2)[1][0]["grid"] == 1
    # generic kernels: dimensions in groups of four
    for D, dims in ((1, [1]), (3, [3]), (4, [4]), (5, [4, 1]), (9, [4, 4, 1]), (12, [4, 4, 4])):
        g = plan(5, D, 8, interior_fixed=2)
        forms, ls = check(emu, g, call(g, 1000, extra=1))
        assert forms[0] == F_GENERIC and [l["dim0"] for l in ls] == [4 * i for i in range(len(dims))]
        assert [l["fn"] for l in ls] == [2000 + 10 * dc + 1 for dc in dims] and ls[0]["grid"] == 16
        ls = check(emu, g, call(g, 1000, update=1))[1]
        assert [l["fn"] for l in ls] == [2100 + 10 * dc for dc in dims] and all(l["block"] == 64 for l in ls)
    assert decide(emu, plan(5, 3, 8, interior_fixed=2, generic=False), KNOBS, 256, call(g, 10))[2]          # no kernel: an error, not a launch
    # the update path: the rolled entry's whole-sector kernel, by phase and cost; without it the staged one
    u = plain()
    assert check(emu, u, call(u, 1000, update=1))[1][0]["fn"] == static_tag("rolled", 20) and (8 * 3 * 10 * 8) % 64 == 0
    u7 = plain(K=7)
    assert check(emu, u7, call(u7, 1000, update=1, extra=1))[1][0]["fn"] == static_tag("rolled", 23)
    assert check(emu, u, call(u, 1000, update=1), no_slab=1)[1][0]["fn"] == static_tag("rolled", 10)
    assert check(emu, dict(u, rolled=rolled(3, upd_slab_lds=65537)), call(u, 1000, update=1, extra=1))[1][0]["fn"] == static_tag("rolled", 11)
    assert check(emu, u, call(u, 10 ** 6, update=1, flags=GENERIC))[1][0]["grid"] == 4096


def test_size_limits(emu):
    """padded16(B) x 8 x max(K, n_fixed x D) >= 2^32 refuses the static dimension-in-lane form; the mixed request checks B itself."""
    p = n10k8()
    per = 8 * max(p["K"], p["n_fixed"] * p["D"])            # 8 x 51
    assert per == 408
    edge = 2 ** 32 // per // 16 * 16                         # largest multiple of 16 that fits
    assert (edge * per < 2 ** 32 <= (edge + 16) * per)
    fits = lambda B, padded: bool(rule(emu, p, 0, B, int(padded)))
    for B, want in ((edge, F_DIMLANE), (edge + 1, F_SLAB)):
        assert form(emu, p, call(p, B, flags=DIMLANE)) == want and fits(B, True) == (want == F_DIMLANE) == offsets_fit(p, B, True)
    # a batch that is no multiple of 16 and fits as it is, but not with its padded rows (a one-dimensional plan: 8 x 17 bytes per row)
    p1 = plan(5, 1, 8, fast=static(1, 8), g1=static(1, 8), dl=dimlane(5, 8, tpw=64, hi=0))
    last = (2 ** 32 - 1) // (8 * 17)
    assert last % 16 == 1 and last * 136 < 2 ** 32 <= pad16(last) * 136
    fits1 = lambda B, padded: bool(rule(emu, p1, 0, B, int(padded)))
    assert fits1(last, False) and not fits1(last, True) and not fits1(last + 1, False) and fits1(last - 1, True)
    assert form(emu, p1, call(p1, last - 1)) == F_DIMLANE and form(emu, p1, call(p1, last)) == F_FUSED


def test_shared_rules(emu):
    p = n10k8()
    assert rule(emu, p, 1, 341, 3) == 1 and rule(emu, p, 1, 342, 3) == 0 and rule(emu, p, 1, 16, 1, cus=4) == 1 and rule(emu, p, 1, 17, 1, cus=4) == 0
    for dims, N, fm in ((3, 10, 4), (1, 10, 4), (4, 10, 2), (3, 12, 5), (1, 8, 3), (2, 2, 0)):
        assert rule(emu, p, 2, dims, N) == stage_lds(dims, N) and rule(emu, p, 3, dims, N, fm) == solve_lds(dims, N, fm)
    assert stage_lds(3, 10) == 64 * 15 * 16 and solve_lds(3, 10, 4) == 2 * 15360 + 2 * 22 * 512


def test_queue(emu):
    p = n10k8()
    kn = dict(KNOBS)

    def q(n, B, layout="soa", flags=0, plan_=p, cus=CUS, **knobs):
        res = []
        for n_cu in cus:
            got = decide_queue(emu, plan_, dict(kn, **knobs), n_cu, n, B, layouts(plan_, B)[layout], flags)
            want = expected_queue(plan_, dict(kn, **knobs), n_cu, n, B, layouts(plan_, B)[layout], flags)
            assert got[:3] == want[:3] and got[3] == want[3], (n_cu, got, want)
            res.append(got)
        return res[0]
    # by total trajectories: 8 x 2016 = 16128
    assert q(8, 2016)[:2] == (1, 1) and q(8, 2017)[:2] == (1, 0) and q(9, 2016)[:2] == (1, 0)
    assert q(8, 2016)[3][0]["fn"] == 3001 and q(8, 2017)[3][0]["fn"] == 1002 and q(8, 2017)[3][0]["attr"] == 3
    assert q(8, 2016, "aos")[:2] == (1, 1) and q(8, 2001, "soa16")[:2] == (1, 1) and q(8, 2016, "strided")[:2] == (1, 0)
    assert q(20, 10000)[3][0]["grid"] == 449 and q(20, 10000)[3][0]["ntiles"] == 3140
    assert q(200, 10000)[:2] == (1, 0) and [l["ntiles"] for l in q(200, 10000)[3]] == [96 * 157, 96 * 157, 8 * 157]
    assert q(200, 10)[:2] == (1, 1) and len(q(200, 10)[3]) == 3 and q(96, 168)[:2] == (1, 1) and q(97, 169)[:2] == (1, 0)
    # flags and options
    assert q(8, 5000, flags=DIMLANE)[:2] == (0, 1) and q(8, 2016, flags=FUSED)[:2] == (1, 0)
    for fl in (GENERIC, SPLIT, ONE_PER_BATCH):
        assert q(8, 2016, flags=fl)[3] == []
    assert q(1, 2016)[3] == [] and q(8, 2016, no_queue=1)[3] == [] and q(8, 2016, no_dimlane=1)[:2] == (1, 0) and q(8, 2016, no_slab=1)[:2] == (0, 1)
    assert q(8, 10 ** 5, no_slab=1)[:2] == (0, 1) and q(8, 2016, "strided", no_slab=1)[3] == []
    assert q(8, 2016, plan_=dict(p, dl=dimlane(5, 8, queue=0)))[:2] == (1, 0)
    assert q(8, 2016, plan_=dict(p, slab=dict(lds=65024, queue=0, extra=1)))[:2] == (0, 1)
    assert q(8, 2017, plan_=dict(p, slab=dict(lds=65024, queue=0, extra=1)))[:2] == (0, 1)      # without a slab alternative: any size
    # the dimension-in-lane grid of the queue: 8 x CUs whatever the option; long chains as single launches
    big = dict(p, slab=None, dl=dimlane(5, 8, hi=0))
    assert q(8, 10 ** 6, plan_=big, dl_grid_per_cu=3)[3][0]["grid"] == 2048 and q(8, 10 ** 6, plan_=big, cus=(4,))[3][0]["grid"] == 32
    ws = dict(p, slab=None, dl=dimlane(6, 32, np_=1, hi=0, ws_per_lane=560))
    l = q(8, 10 ** 6, plan_=ws)[3][0]
    assert l["grid"] == 512 and l["ws_bytes"] == 560 * 512 * 128
    # tiles of a launch in 32 bits: tiles per batch x batches per launch < 2^31 (sizes that exist only here)
    B = 64 * (2 ** 31 // 96) + 1                     # 22369622 tiles x 96 >= 2^31
    assert q(96, B - 1, flags=FUSED)[:2] == (1, 0) and q(96, B, flags=FUSED)[3] == [] and q(95, B, flags=FUSED)[:2] == (1, 0)
    # (the dimension-in-lane twin of this limit cannot be reached: the 32-bit offsets allow B < 2^32 / 16 at best, and tiles hold 16
    # trajectories or more -- 96 x 2^24 tiles)
    assert q(96, 2 ** 28 - 16, plan_=dict(p, slab=None))[3] == []


if __name__ == "__main__" and "--dump" in sys.argv:
    # one line per case for the stand-alone build of tests/launch_plan_emu.cpp (-DMTG_LAUNCH_PLAN_EMU_MAIN): the calls and queues of
    # the case list above, recorded by running the tests against a stub that writes instead of deciding
    lines = []

    class Recorder:
        def __init__(self, lib):
            self.lib = lib

        def __getattr__(self, name):
            real = getattr(self.lib, name)
            if name == "mtg_launch_rule_emu":
                return real

            def wrapped(plan_p, knobs_p, n_cu, tail_p, max_launches, out_p):
                n_tail = 14 if name == "mtg_launch_plan_emu" else 11
                ints = [plan_p[i] for i in range(78)] + [knobs_p[i] for i in range(14)] + [tail_p[i] for i in range(n_tail)]
                lines.append(" ".join(str(v) for v in [0 if n_tail == 14 else 1, n_cu] + ints))
                return real(plan_p, knobs_p, n_cu, tail_p, max_launches, out_p)
            return wrapped
    lib = Recorder(load_emu())
    for name, fn in sorted(globals().items()):
        if name.startswith("test_"):
            fn(lib)
    print("\n".join(lines))
