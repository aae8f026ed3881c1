"""Plan.launch_form over the matrix of tests/golden/launch_forms.json (tools/record_launch_forms.py: N = 8 / 10 / 12 with eight chain
lengths, config 5's shape, a ragged mask in 1 / 3 / 4 / 5 dimensions; batches either side of every edge of the decision; layouts,
forced forms, extra outputs).  The file was recorded on the commit before the launch decision moved into csrc/mtg_launch_plan.h,
when the report was a hand-written copy of the launcher's rules: the decision the launcher now runs must answer the same.  Host
calls only, nothing is launched."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_launch_forms_match_the_recorded_matrix():
    import torch
    import mav_trajectory_generation_amd as m
    with open(os.path.join(ROOT, "tests", "golden", "launch_forms.json")) as fh:
        golden = json.load(fh)
    # the thresholds scale with the CU count: another device needs its own recording (a failure, not a skip)
    assert torch.cuda.get_device_properties(0).multi_processor_count == golden["cu_count"]
    ctx = m.Context(0)
    for name, value in golden["options"].items():
        ctx.set_option(name, value)
    n_cases, wrong = 0, []
    for s in golden["plans"]:
        plan = m.Plan(ctx, s["n"], s["d"], s["k"], s["deriv"], s["mask"])
        assert len(s["forms"]) == len(golden["cases"])
        for (batch, layout, dims, extra), code in zip(golden["cases"], s["forms"]):      # one report-code digit per case
            got, form = plan.launch_form(batch, layout, dims, extra_outputs=bool(extra)), golden["codes"][int(code)]
            n_cases += 1
            if got != form:
                wrong.append((s["n"], s["d"], s["k"], batch, layout, dims, extra, form, got))
        plan.close()
    ctx.close()
    assert n_cases >= 300 and set("".join(s["forms"] for s in golden["plans"])) == set("01234567")      # every form code occurs
    assert not wrong, wrong[:20]
