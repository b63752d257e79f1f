"""EVERY feature-level kernel instantiation (the 78 rows of feature_kernel_cases.py) UNDER INSTANCE SCHEDULING, and the drivers above them.

Beyond one wavefront per SIMD every solve kernel works on instance p.order[blockIdx.x] instead of instance blockIdx.x, and everything a batch carries
per instance -- reference rows and offsets, the derived parameter tables, mask words, bounds table, slack schedule, accumulators, episode words,
noise -- must be indexed with that instance and never with the slot.  A slot index stays in bounds: it reads a valid row of a valid array, so no
guard band or status code notices; only a batch that IS scheduled, whose rows are all different problems, does.  test_gpu_every_feature_kernel.py
runs twelve instances, which the scheduler never deals; here the same twelve judged instances are embedded (feature_kernel_cases.embed) in a batch
just beyond one wavefront per SIMD -- its size found by asking the library (feature_loop.smallest_scheduled_batch) -- among fillers with feature
rows of their own.  Per kernel, with scheduling on and off, each on a fresh handle and stream: the name asserted, a priming solve (so that the
measured launch has an order), everything restored, then the fused step of test_gpu_every_feature_kernel.py with every optional output wired.
  conditions (scheduling on): the order at the measured launch is a permutation, not the identity, and moves 8 or more of the 11 live judged instances;
  the judged rows: test_gpu_every_feature_kernel.py's _placement, _against_oracle and _bookkeeping, unchanged, against the case's own inputs;
  the whole batch: every output bit for bit the same with scheduling on and off (one instance per wavefront or workgroup: DESIGN.md section 4),
  bands intact, inputs and feature arrays unchanged, one offset increment per instance that stepped, accumulators consistent, idle instances untouched.
The drivers: fused_loop on a scheduled handle (the order then comes from the handle's own iteration counts), PipelinedMpc with scheduling at its
default on both sub-handles, and a seed sweep with per-seed tables, each against the same run unscheduled, bit for bit."""
import numpy as np
import pytest

import feature_kernel_cases as fk
from feature_loop import FeatureStack, fused_loop, make, mg, on_own_stream, smallest_scheduled_batch, smooth_path
from helpers import random_batch
from instance_bounds_cases import draw_bounds, per_instance
from test_gpu_every_feature_kernel import OUTPUTS, _against_oracle, _bookkeeping, _launches, _nan_launch_is_the_first, _placement, _schedule_of

pytestmark = pytest.mark.gpu
B = fk.B
MIN_MOVED = 8            # of the 11 live judged instances: a condition on the inputs, not a measurement
FLOATS = ("x0", "obst", "X", "U", "u0", "cost", "margin")
_EMBEDDED = {}


def _embedded(orc, case, inp, alpha, Bs, pos):
    """the case's scheduled batch, once per (inputs, batch size) and session: cases that differ in the lane mapping alone share it.  Not to be written to"""
    key = (case["N"], case["no"], case["level"], alpha is not None, Bs)
    if key not in _EMBEDDED:
        _EMBEDDED[key] = fk.embed(orc, inp, Bs, pos, alpha=alpha)
    return _EMBEDDED[key]


def order_facts(order, Bs, judged):
    """(why not, how many of `judged` run in a slot that is not their index, the largest |slot - index| over the batch) of the permutation in effect:
    slot s runs instance order[s]"""
    if order is None:
        return ["no order in effect at the measured launch"], 0, 0
    if not np.array_equal(np.sort(order), np.arange(Bs)):
        return ["the order is no permutation"], 0, 0
    slot = np.argsort(order)
    moved = int((slot[judged] != judged).sum())
    why = []
    if np.array_equal(order, np.arange(Bs)): why.append("the order is the identity")
    if moved < MIN_MOVED: why.append(f"{moved} of {len(judged)} live judged instances moved")
    return why, moved, int(np.abs(slot - np.arange(Bs)).max())


def _whole_batch(emb, on, off, why, what=""):
    """everything that holds for all Bs rows, fillers included"""
    Bs = emb["Bs"]
    for k in OUTPUTS:
        if not np.array_equal(on[k], off[k], equal_nan=k in FLOATS): why.append(f"{what}{k} differs between scheduling on and off in rows {np.nonzero((on[k] != off[k]).reshape(Bs, -1).any(axis=1))[0][:8].tolist()}")
    stepped = emb["ep_flags"] == 0
    idle = ~stepped
    for tag, r in (("on", on), ("off", off)):
        if not r["intact"]: why.append(f"{what}{tag}: a guard band was written")
        if r["written"]: why.append(f"{what}{tag}: written by the launch: {r['written']}")
    r = on
    if not np.array_equal(r["offset"], emb["offset"] + stepped): why.append(f"{what}reference offsets: rows {np.nonzero(r['offset'] != emb['offset'] + stepped)[0][:8].tolist()}")
    if not np.isin(r["status"][stepped], (0, 2, 4)).all(): why.append(f"{what}status values {sorted(set(r['status'][stepped].tolist()))}")
    if not np.array_equal(r["iacc"][stepped], 1000 + r["iters"][stepped]): why.append(f"{what}iteration accumulator")
    if not np.array_equal(r["sacc"][stepped], ((r["status"] == 4) + 65536 * (r["status"] == 2))[stepped]): why.append(f"{what}status accumulator")
    if not np.array_equal(r["steps"][stepped], (100 + ((r["flags"] & 1) == 0))[stepped]): why.append(f"{what}step counters")
    init = dict(x0=emb["x0"], obst=r["obst_in"], X=r["X0"], U=r["U0"], u0=np.full((Bs, 2), -5.0), cost=np.full(Bs, -5.0), margin=np.full(Bs, np.inf),
                status=np.full(Bs, -9), iters=np.full(Bs, -9), flags=emb["ep_flags"], steps=np.full(Bs, 100), iacc=np.full(Bs, 1000), sacc=np.zeros(Bs, int),
                offset=emb["offset"])
    for k, v in init.items():
        if not np.array_equal(r[k][idle], v[idle], equal_nan=(k == "obst")): why.append(f"{what}an idle instance's {k} was written")


ROWS = OUTPUTS + ("X0", "U0", "obst_in")


def _judged(r, pos):
    """rows pos of everything a launch returned: what _placement, _against_oracle and _bookkeeping see, in the case's own numbering"""
    return dict(r, **{k: r[k][pos] for k in ROWS})


def _body(mg, family, level, schedule_of=None):
    import torch
    mpc_gpu, orc = mg
    Bs = smallest_scheduled_batch(mpc_gpu)
    pos = fk.positions(Bs)
    cases = fk.cases_of(family, level)
    bad, ran = [], []
    for case in cases:
        inp, alpha = (fk.inputs(orc, case), None) if schedule_of is None else schedule_of(orc, case)
        emb = _embedded(orc, case, inp, alpha, Bs, pos)
        runs = {}
        for on in (True, False):
            with torch.cuda.stream(torch.cuda.Stream()):      # a fresh handle on a stream of its own per run
                runs[on] = _launches(mpc_gpu, torch, case, emb, level >= 3, emb.get("alpha") if alpha is not None else None, scheduling=on, prime=True)
        r, r_off = runs[True][0], runs[False][0]
        ran.append(r["name"])
        live = pos[inp["ep_flags"] == 0]
        why, moved, far = order_facts(r["order"], Bs, live)
        for other in runs[True][1:]:
            why += order_facts(other["order"], Bs, live)[0]
        if any(o["order"] is not None for o in runs[False]): why.append("an order in effect with scheduling off")
        rep = dict(converged=0, adjudicated=0, status_borderline=0, worst_gpu_oracle=0.0, worst_gpu_exact=0.0)
        _whole_batch(emb, r, r_off, why)
        j = _judged(r, pos)
        _placement(inp, j, why)
        _against_oracle(orc, inp, j, why, rep, alpha)
        _bookkeeping(orc, inp, j, why)
        if level >= 3:
            again, again_off = runs[True][1], runs[False][1]
            _whole_batch(emb, again, again_off, why, "second launch: ")
            _nan_launch_is_the_first(emb, r, again, why, nan_ok=FLOATS)
        print(f"FEATURE-KERNEL scheduled{'' if alpha is None else ' with a slack schedule'} {r['name']} N {case['N']} n_obst {case['no']} Bs {Bs}: moved {moved} of {len(live)} "
              f"farthest {far} converged {rep['converged']} of {B - 1} worst_gpu_oracle {rep['worst_gpu_oracle']:.3e} "
              f"adjudicated {rep['adjudicated']} worst_gpu_exact {rep['worst_gpu_exact']:.3e} status_borderline {rep['status_borderline']} "
              f"status {j['status'].tolist()} fillers with status 0 / 2 / 4 {[int((r['status'][emb['filler']] == v).sum()) for v in (0, 2, 4)]} "
              f"{'FAILED: ' + '; '.join(why) if why else 'ok'}")
        if why:
            bad.append((case["name"], why))
    assert not bad, bad
    assert sorted(ran) == sorted(c["name"] for c in cases), ran      # nothing refused, nothing skipped


@pytest.mark.parametrize("level", fk.LEVELS)
@pytest.mark.parametrize("family", fk.FAMILIES)
def test_every_feature_instantiation_under_instance_scheduling(mg, family, level):
    on_own_stream(_body, mg, family, level)


@pytest.mark.parametrize("family", fk.FAMILIES)
def test_level_four_with_an_explicit_slack_schedule_under_instance_scheduling(mg, family):
    """the schedule of world "own" (slack_schedule_cases.feature_problem) on the judged rows, a row of their own on every filler: alpha[inst][stage]"""
    on_own_stream(_body, mg, family, 4, _schedule_of("own"))


# ---------------------------------------------------------------------------------------------------------------- the drivers above the kernels
LOOP_SHAPES = {"split": (20, 3), "one": (50, 3), "wide": (20, 20)}      # the smallest horizon of feature_kernel_cases.HORIZON per family
assert all(N == min(n for (f, _), n in fk.HORIZON.items() if f == fam) for fam, (N, _) in LOOP_SHAPES.items())
LOOP_KERNEL = {"split": "rti_split_kernel<3, 3,", "one": "rti_solve_kernel<3, 64,", "wide": "rti_wide_kernel<20, 2,"}


def loop_inputs(N, no, Bs, seed, steps):
    """the full FeatureStack for Bs instances: weights, radii, a mask pair and a bounds pair that switch halfway, an advancing reference"""
    rng = np.random.default_rng(seed)
    x0, goal, obst = random_batch(Bs, no, seed=seed)
    x0[:, 3:] = 0.0
    masks = []
    for _ in range(2):
        m = rng.uniform(size=(Bs, no)) < 0.6
        m[np.arange(Bs), rng.integers(0, no, Bs)] = True
        masks.append(m)
    bounds = tuple(per_instance(draw_bounds(rng, Bs, Bs + 1)[0], np.arange(1, Bs + 1)) for _ in range(2))
    stack = FeatureStack(W=np.array(fk.IP["W"]) * rng.uniform(0.5, 3.0, (Bs, 6)), We=np.array(fk.IP["We"]) * rng.uniform(0.5, 3.0, (Bs, 4)),
                         r_safe=rng.uniform(1.6, 3.0, (Bs, no)), mask=tuple(masks), bounds=bounds, path=smooth_path(rng, Bs, steps + N + 1))
    return stack, x0, goal, obst


def _fused_loop(mg, family):
    mpc_gpu, _ = mg
    N, no = LOOP_SHAPES[family]
    Bs, steps = smallest_scheduled_batch(mpc_gpu), 6
    stack, x0, goal, obst = loop_inputs(N, no, Bs, 2100 + N + no, steps)
    res, orders = {}, {}
    for on in (True, False):
        with make(mpc_gpu, N, no, Bs, scheduling=on) as s:
            res[on] = fused_loop(mpc_gpu, N, no, Bs, steps, x0, goal, obst, stack, handle=s)
            assert s.kernel_name(Bs).startswith(LOOP_KERNEL[family]) and s.kernel_name(Bs).endswith(", true" * 4 + ">"), s.kernel_name(Bs)
            orders[on] = s.instance_order(Bs)
    assert orders[False] is None
    order = orders[True]      # built from the handle's own iteration counts: the loop wires no `iters`
    assert order is not None and np.array_equal(np.sort(order), np.arange(Bs)) and not np.array_equal(order, np.arange(Bs))
    far = int(np.abs(np.argsort(order) - np.arange(Bs)).max())
    print(f"FEATURE-LOOP scheduled {family} N {N} n_obst {no} Bs {Bs}: farthest {far}, instances at their own index {int((order == np.arange(Bs)).sum())}, "
          f"goal reached by {int((res[True]['fl'] & 1).sum())}")
    for k in res[True]:
        assert np.array_equal(res[True][k], res[False][k]), k
    assert not np.array_equal(res[True]["X"], np.zeros_like(res[True]["X"]))


@pytest.mark.parametrize("family", list(LOOP_SHAPES))
def test_fused_loop_with_the_full_stack_under_instance_scheduling(mg, family):
    on_own_stream(_fused_loop, mg, family)


def _pipelined(mg):
    """test_pipelined_sub_batches_equal_one_handle (test_gpu_instance_bounds.py) at 2 Bs + 1 instances, scheduling left at its default on both
    sub-handles: every sub-batch is one the scheduler deals"""
    from mpc_gpu.pipeline import PipelinedMpc
    mpc_gpu, _ = mg
    N, no, steps = 20, 3, 6
    Bs = smallest_scheduled_batch(mpc_gpu)
    Bp = 2 * Bs + 1
    stack, x0, goal, obst = loop_inputs(N, no, Bp, 3013, steps)
    one = fused_loop(mpc_gpu, N, no, Bp, steps, x0, goal, obst, stack)            # one unscheduled handle
    with PipelinedMpc(N, no, 0.1 * N, max_batch=Bp, streams=2) as p:
        two = fused_loop(mpc_gpu, N, no, Bp, steps, x0, goal, obst, stack, solver=p)
        assert p.kernel_name().endswith(", true" * 4 + ">")
        for lo, hi, m, _ in p.parts:
            order = m.instance_order(hi - lo)
            assert hi - lo >= Bs and order is not None and np.array_equal(np.sort(order), np.arange(hi - lo)) and not np.array_equal(order, np.arange(hi - lo))
    for k in one:
        assert np.array_equal(one[k], two[k]), k


def test_pipelined_sub_batches_under_instance_scheduling(mg):
    on_own_stream(_pipelined, mg)


def _seed_sweep(built):
    import mpc_gpu
    import sweep_cases as sc
    import sweep_feature_cases as fc
    mpc_gpu.BatchedMpc.default_lanes_per_stage = 0
    Bs = smallest_scheduled_batch(mpc_gpu)
    count = Bs + 40
    a = fc.arrays(count)
    traced = [0, 7, Bs - 1, Bs, count - 1]
    res, orders = {}, {}
    for on in (True, False):
        with mpc_gpu.BatchedMpc(max_batch=Bs, **sc.PROBLEM) as m:
            m.set_instance_scheduling(on)
            res[on] = mpc_gpu.run_seed_sweep(sc.START, sc.GOAL, "RANDOM", (0, count), Bs, solver=m, max_iter=8, r_safe=a["r_safe"], active=a["active"],
                                             bounds=a["bounds"], status_log=True, trace=traced, trace_pred=False)
            orders[on] = m.instance_order(Bs)
    assert orders[False] is None
    order = orders[True]
    assert order is not None and np.array_equal(np.sort(order), np.arange(Bs)) and not np.array_equal(order, np.arange(Bs))
    r, u = res[True], res[False]
    print(f"SEED-SWEEP scheduled slots {Bs} seeds {count}: steps_run {r['steps_run']}, farthest {int(np.abs(np.argsort(order) - np.arange(Bs)).max())}, "
          f"status2 {int(r['status2'].sum())} status4 {int(r['status4'].sum())}")
    assert np.array_equal(r["table"], u["table"]), np.nonzero((r["table"] != u["table"]).any(axis=1))[0]
    assert np.array_equal(r["x_last"], u["x_last"])
    for n in ("status2", "status4", "first_bad"):
        assert np.array_equal(r[n], u[n]), n
    assert r["steps_run"] == u["steps_run"] and r["solves"] == u["solves"]
    for k in traced:      # the per-seed rows the device recorded through slot_state: the slot every seed ran in, step by step
        for n in r["trace"][k]:
            assert np.array_equal(r["trace"][k][n], u["trace"][k][n]), (k, n)
    assert r["solves"] > 8 * Bs      # (more solves than one round of the slots holds: seeds started in refilled slots)


def test_seed_sweep_with_per_seed_tables_under_instance_scheduling(built):
    on_own_stream(_seed_sweep, built)
