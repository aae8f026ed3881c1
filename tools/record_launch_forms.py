"""Records tests/golden/launch_forms.json: what Plan.launch_form answers over a matrix of shapes, batches, layouts, forced forms and
extra outputs, on this device.  Public Python API only, so the same script runs on any commit: the golden file is taken on the
commit BEFORE a change to the launch decision, and tests/test_gpu_launch_form_matrix.py holds the next one to it.
usage: record_launch_forms.py OUT.json [PACKAGE_ROOT]   (PACKAGE_ROOT: a tree holding mav_trajectory_generation_amd/, default: this one)"""
import json
import os
import sys


# Either side of every edge of the decision at 256 CUs: the row-cooperative range (1024 / 2048 trajectories), 1.5 dimension-in-lane
# workgroups per CU (16128 at 42 trajectories per workgroup), the N = 12 / K = 32 extra-output exception (20000), 4 x CUs split-form
# workgroups (341 tiles x 3 dimensions; 1024 tiles), 8 dimension-in-lane workgroups per CU at 16 trajectories per wave (65536).
BATCHES = [1, 63, 1024, 1025, 2048, 2049, 16128, 16129, 20000, 20001, 21824, 21825, 65536, 65537, 131072]
EXTRA_BATCHES = [1000, 16128, 16129, 20000, 20001, 100000]
FORCED = [(1000, "soa"), (50000, "aos"), (1001, "soa16")]


def shapes():
    out = [dict(n=n, d=3, k=k, deriv=n // 2 - 1, mask=[(1 << n // 2) - 1] + [1] * (k - 1) + [(1 << n // 2) - 1])
           for n in (8, 10, 12) for k in (2, 4, 8, 16, 17, 32, 50, 100)]
    out.append(dict(n=10, d=4, k=16, deriv=4, mask=[31] + [7] * 15 + [31]))       # config 5
    out += [dict(n=10, d=d, k=6, deriv=4, mask=[31, 1, 3, 1, 7, 1, 31]) for d in (1, 3, 4, 5)]      # a ragged mask: generic kernels
    return out


def cases():
    out = [(b, "soa", "auto", False) for b in BATCHES]
    out += [(b, "soa", "auto", True) for b in EXTRA_BATCHES]
    out += [(b, "aos", "auto", False) for b in (1024, 16128, 16129, 65537)]
    out += [(b, lay, dims, extra) for dims in ("fused", "split", "dimlane", "coop") for (b, lay) in FORCED for extra in ((False, True) if lay == "soa" else (False,))]
    out += [(1001, "soa16", "auto", False), (16127, "soa16", "auto", False), (16145, "soa16", "auto", False)]
    return out


CODES = ["generic", "fused", "split", "rolled", "slab", "dimlane", "dimlane_rt", "coop"]      # the report codes 0 .. 7


def write(path, cu_count, plans):
    """plans: [shape dict + forms (one report-code digit per case of cases(), in order)]."""
    head = {"cu_count": cu_count, "options": {"coop": -1}, "codes": CODES, "case_fields": ["batch", "layout", "dims", "extra_outputs"],
            "cases": [[b, lay, dims, int(extra)] for (b, lay, dims, extra) in cases()]}
    with open(path, "w") as fh:
        fh.write("{\n" + ",\n".join(' "%s": %s' % (k, json.dumps(v)) for k, v in head.items()))
        fh.write(',\n "plans": [\n' + ",\n".join("  " + json.dumps(p) for p in plans) + "\n ]\n}\n")


def main():
    root = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    import mav_trajectory_generation_amd as m
    assert os.path.abspath(m.__file__).startswith(root), m.__file__
    ctx = m.Context(0)
    ctx.set_option("coop", -1)      # the shipped default range, whatever MTG_COOP says
    plans = []
    for s in shapes():
        plan = m.Plan(ctx, s["n"], s["d"], s["k"], s["deriv"], s["mask"])
        forms = "".join(str(CODES.index(plan.launch_form(b, lay, dims, extra_outputs=extra))) for (b, lay, dims, extra) in cases())
        plan.close()
        plans.append(dict(s, forms=forms))
    cu_count = torch.cuda.get_device_properties(0).multi_processor_count
    write(sys.argv[1], cu_count, plans)
    print("recorded", sum(len(p["forms"]) for p in plans), "cases of", len(plans), "plans at", cu_count, "CUs")
    ctx.close()


if __name__ == "__main__":
    main()
