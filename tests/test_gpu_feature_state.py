"""The host-side state of the per-instance features (per-stage reference, instance parameters, obstacle mask, instance bounds, SQP loop, slack schedule)
on the GPU: a handle walked through the features in any order is, after every transition, a fresh handle configured directly into the same state -- the
same kernel, the same solve bit for bit; the handle's default companions survive the caller's values; handles are created, used and destroyed repeatedly.
The smallest shapes that reach every level's kernel: N = 6, batch 4, 3 obstacles (the stage-split family) and 12 (the multi-wavefront family)."""
import numpy as np
import pytest

from feature_loop import assert_same, make, mg, on_own_stream, run, smooth_path
from helpers import random_batch
from instance_bounds_cases import draw_bounds, per_instance
from obstacle_mask_cases import draw_masks

pytestmark = pytest.mark.gpu

N, B = 6, 4
FAMILIES = [(3, "rti_split_kernel"), (12, "rti_wide_kernel")]
ORDER = ("ref", "ip", "om", "bd", "sqp", "alpha")      # the order a fresh handle is configured in


class Case:
    """the inputs of one family and one value per feature and form, drawn once; the device tensors stay alive with it"""

    def __init__(self, mpc_gpu, no):
        import torch
        self.mpc_gpu, self.no = mpc_gpu, no
        rng = np.random.default_rng(900 + no)
        self.x0, self.goal, self.obst = random_batch(B, no, seed=77 + no)
        tt = lambda a: torch.tensor(np.ascontiguousarray(a), device=torch.device("cuda", 0))
        with make(mpc_gpu, N, no, B) as s:
            W, We = np.array(list(s.cfg.W)), np.array(list(s.cfg.We))
            menu, group = draw_bounds(rng, B)
            bounds = per_instance(menu, group)
            table = mpc_gpu.pack_instance_bounds(s.cfg, B, **bounds)
        par = dict(W=W * rng.uniform(0.5, 2.0, (B, 6)), We=We * rng.uniform(0.5, 2.0, (B, 4)), r_safe=rng.uniform(2.0, 2.8, (B, no)))
        mask = draw_masks(rng, B, no)
        self.value = {
            ("ref", "host"): smooth_path(rng, B, N + 1),
            ("ip", "host"): par, ("ip", "dev"): {k: tt(v) for k, v in par.items()},
            ("om", "host"): mask, ("om", "dev"): tt(mpc_gpu.pack_obstacle_mask(mask).view(np.int32)),
            ("bd", "host"): bounds, ("bd", "dev"): tt(table),
            ("sqp", "host"): 2,
            ("alpha", "host"): rng.uniform(10.0, 1000.0, (B, N + 1)),
        }
        torch.cuda.synchronize()

    def set(self, s, feature, form):
        """one transition: `feature` on in the host or the device form, or off (form None)"""
        v = None if form is None else self.value[feature, form]
        if feature == "ref":
            s.set_reference(v)
        elif feature == "ip":
            s.set_instance_params(**(v or {}))
        elif feature == "om":
            s.set_obstacle_mask(v)
        elif feature == "bd":
            if form == "dev":
                s.set_instance_bounds_dev(v)
            else:
                s.set_instance_bounds(**(v or {}))
        elif feature == "sqp":
            s.set_sqp(v or 1, 0.0)
        else:
            s.set_slack_schedule(v)

    def fresh(self, state):
        s = make(self.mpc_gpu, N, self.no, B)
        for feature in ORDER:
            if state.get(feature):
                self.set(s, feature, state[feature])
        return s

    def solve(self, s):
        return run(s, self.x0, self.obst, self.goal, steps=1)


# (feature, form): on in that form, or off (None).  The three sequences the per-feature tests do not cover, then everything on and off in the reverse
# order, and everything on in the other forms and off in the same order
WALK = [("ip", "host"), ("om", "host"), ("ip", None), ("om", None),
        ("ip", "dev"), ("bd", "dev"), ("ip", None), ("sqp", "host"), ("bd", None), ("sqp", None),
        ("ref", "host"), ("ip", "host"), ("om", "dev"), ("bd", "host"), ("sqp", "host"), ("alpha", "host"),
        ("alpha", None), ("sqp", None), ("bd", None), ("om", None), ("ip", None), ("ref", None),
        ("ref", "host"), ("ip", "dev"), ("om", "host"), ("bd", "dev"), ("sqp", "host"), ("alpha", "host"),
        ("ref", None), ("ip", None), ("om", None), ("bd", None), ("sqp", None), ("alpha", None)]


def _body_walk(mg, no, family):
    mpc_gpu, _ = mg
    c = Case(mpc_gpu, no)
    state, names = {}, set()
    with make(mpc_gpu, N, no, B) as s:
        for k, (feature, form) in enumerate(WALK):
            c.set(s, feature, form)
            state[feature] = form
            with c.fresh(state) as f:
                name = s.kernel_name(B)
                assert name == f.kernel_name(B) and name.startswith(family), (k, feature, form, name, f.kernel_name(B))
                out = c.solve(s)
                assert_same(out, c.solve(f))
            print(k, feature, form, "status", out[0][4].tolist(), "iters", out[0][5].tolist())
            assert (out[0][4] != 4).any(), (k, feature, form)      # (something was solved)
            names.add(name)
    assert not any(state.values())
    assert len(names) == 6, names      # the walk went through every feature level's kernel
    print(no, "obstacles:", len(WALK), "transitions,", sorted(names))


@pytest.mark.parametrize("no,family", FAMILIES)
def test_any_order_of_switching_is_a_fresh_handle(mg, no, family):
    on_own_stream(_body_walk, mg, no, family)


def _body_defaults(mg, no, form):
    mpc_gpu, _ = mg
    c = Case(mpc_gpu, no)
    with make(mpc_gpu, N, no, B) as s:
        c.set(s, "om", "host")
        a = c.solve(s)
        c.set(s, "ip", form)
        c.solve(s)
        c.set(s, "ip", None)
        b = c.solve(s)
    assert_same(a, b)


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("no", [no for no, _ in FAMILIES])
def test_defaults_are_not_overwritten(mg, no, form):
    on_own_stream(_body_defaults, mg, no, form)


def _body_repeats(mg):
    mpc_gpu, _ = mg
    c = Case(mpc_gpu, 3)
    everything = dict(ref="host", ip="dev", om="host", bd="dev", sqp="host", alpha="host")
    outs = []
    for _ in range(9):
        with c.fresh(everything) as s:
            outs.append(c.solve(s))
    assert_same(outs[0], outs[-1])


def test_create_use_destroy_repeats(mg):
    """no leak detector: it shows that the handle's memory is released in an order nothing objects to, eight times over"""
    on_own_stream(_body_repeats, mg)
