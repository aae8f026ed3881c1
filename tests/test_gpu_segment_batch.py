"""The device form of the per-segment batch calls (mav_trajectory_generation_amd/segment_checks.py) at B x K = 5 x 3, N = 10: every
wrapper with all its want_* flags off and on (what both runs return is bit-equal, the rest is None), and the inputs the layer must
reject -- float32 times, times on the host, one time too few, [K][B] times shaped [B][K], planes / obstacles on the host.  Those
are rejected in Python before anything is launched: after each, ctx.sync() and a valid call return what they returned before."""
import numpy as np
import pytest

import mav_trajectory_generation_amd as m
from test_gpu_segment_frame import inputs, to_device

pytestmark = pytest.mark.gpu

B, K, N = 5, 3, 10
CONSTRAINTS = dict(f_min=5.0, f_max=14.0, v_max=3.4, omega_xy_max=0.8, omega_z_max=3.0, omega_z_dot_max=5.0)


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = m.Context(0)
    yield c
    c.close()


def planes():
    return m.bounding_box_half_planes([0.1, -0.1, 0.0], [2.6, 2.8, 3.0])


def obstacles():
    return m.sphere_obstacles([[0.5, 0.0, 0.2], [-1.0, 1.0, 0.0]], [0.3, 0.5])


def sampled(out):
    return out if isinstance(out, tuple) else (out, None)


# name -> (D, the want_* flags, call(ctx, coeffs, times, layout, extra, **flags) -> a tuple of tensors and None, the extra input)
WRAPPERS = {
    "sample_range": (3, ("want_valid",), lambda c, co, t, lay, x, **kw: sampled(m.sample_range(c, co, t, 0.0, 0.05, 7, 3, times_layout=lay, **kw)), None),
    "minmax_magnitude": (3, (), lambda c, co, t, lay, x: m.minmax_magnitude(c, co, t, 1, times_layout=lay), None),
    "minmax_axes": (3, ("want_trajectory",), lambda c, co, t, lay, x, **kw: m.minmax_axes(c, co, t, 0, 3, times_layout=lay, **kw), None),
    # (in place on coeffs and times: on copies)
    "scale_segment_times_to_meet_constraints":
        (3, (), lambda c, co, t, lay, x: m.scale_segment_times_to_meet_constraints(c, co.clone(), t.clone(), 1.0, 1.5, times_layout=lay)[:2], None),
    "check_input_feasibility":
        (4, ("want_segments", "want_bounds"),
         lambda c, co, t, lay, x, **kw: m.check_input_feasibility(c, co, t, m.InputConstraints(**CONSTRAINTS), times_layout=lay, **kw), None),
    "check_input_feasibility_recursive":
        (4, ("want_segments", "want_bounds", "want_sections"),
         lambda c, co, t, lay, x, **kw: m.check_input_feasibility_recursive(c, co, t, m.InputConstraints(**CONSTRAINTS), times_layout=lay, **kw), None),
    "check_half_plane_feasibility":
        (3, ("want_clearance",), lambda c, co, t, lay, x, **kw: m.check_half_plane_feasibility(c, co, t, x, times_layout=lay, **kw), planes),
    "check_obstacle_clearance":
        (3, ("want_clearance",), lambda c, co, t, lay, x, **kw: m.check_obstacle_clearance(c, co, t, x, 0.1, times_layout=lay, **kw), obstacles),
    "magnitude_soft_cost":
        (3, (), lambda c, co, t, lay, x: m.magnitude_soft_cost(c, co, t, m.TimeObjectiveParams(constraints=[(1, 2.0), (2, 3.0)]), times_layout=lay), None),
}


def on_host(out):
    return [None if o is None else o.cpu().numpy() for o in out]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_want_flags_and_rejected_inputs(ctx, name):
    import torch
    d, flags, call, make_extra = WRAPPERS[name]
    coeffs, times = inputs(B, K, d, N)
    co, tt = to_device(coeffs, times)
    tt_soa = tt.t().contiguous()
    extra = None if make_extra is None else to_device(make_extra())[0]

    full = on_host(call(ctx, co, tt, "aos", extra, **{f: True for f in flags}))
    assert all(o is not None for o in full) and all(o.shape[0] == B for o in full)
    least = on_host(call(ctx, co, tt, "aos", extra, **{f: False for f in flags}))
    assert len(least) == len(full)
    assert sum(o is None for o in least) >= len(flags)                     # (one flag can stand for several outputs)
    assert all(o is None or same(o, f) for o, f in zip(least, full))
    assert all(same(o, f) for o, f in zip(on_host(call(ctx, co, tt_soa, "soa", extra, **{f: True for f in flags})), full))

    def still_as_before():
        ctx.sync()
        assert all(same(o, f) for o, f in zip(on_host(call(ctx, co, tt, "aos", extra, **{f: True for f in flags})), full))

    rejected = [("float32 times", co, tt.float(), "aos", extra), ("times on the host", co, tt.cpu(), "aos", extra),
                ("one time too few", co, tt.reshape(-1)[:B * K - 1], "aos", extra), ("[K][B] times shaped [B][K]", co, tt, "soa", extra)]
    if extra is not None:
        rejected.append(("planes / obstacles on the host", co, tt, "aos", extra.cpu()))
    for what, c, t, layout, x in rejected:
        with pytest.raises(m.MtgError):
            call(ctx, c, t, layout, x)
            pytest.fail(what + " was accepted")
        still_as_before()
