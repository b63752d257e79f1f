"""EVERY feature-level kernel instantiation (REF, IPAR, OSEL, IBND: the 78 rows of feature_kernel_cases.py) through one guard-banded fused step.

test_gpu_every_kernel.py is the level-0 sweep (a correct source once compiled into a kernel that wrote through a wrong output
pointer); this is the same net under the levels that carry up to six more trailing kernel-argument pointers and spill the most.  Per kernel: a fresh
handle on a stream of its own, its name asserted before anything is launched, every array the launch can touch -- the feature arrays in their
device forms included -- carved out of one sentinel-filled buffer, one fused step with every optional output wired, then
  1. placement: bands intact, the inputs and feature arrays bit for bit what was uploaded, the reference offset advanced for exactly the instances that
     stepped, accumulators and episode words, the idle instance untouched;
  2. the solve against the oracle, group by group (helpers.judge_against_oracle unchanged; the groups carry feature values of their own);
  3. plant step, obstacle motion, margin and flags against the oracle's functions and feature_loop.step_bookkeeping;
  4. levels 3 and 4: the same step again with NaN in the absent obstacles' entries, bit for bit the first (an absent obstacle's own row comes out as
     (NaN, NaN, -vmax, -vmax): IEEE fmax / fmin in the noise clamp return the other operand of a NaN).
No tolerance here is wider than judge_against_oracle's and DESIGN.md section 2's."""
import numpy as np
import pytest

import feature_kernel_cases as fk
from feature_loop import Banded, cfg_values, make, mg, on_own_stream, step_bookkeeping
from helpers import allowed_adjudications, judge_against_oracle, oracle_reference

pytestmark = pytest.mark.gpu
B = fk.B
RANDOMNESS, VMAX = 0.1, 2.0      # the obstacle motion's noise scale and speed limit, as the fused step is given them


def _launches(mpc_gpu, torch, case, inp, nan_absent_too, alpha=None, scheduling=False, prime=False):
    """one fused step of the case's kernel on banded arrays -- and, nan_absent_too, the same step again on the same handle with NaN in the absent
    obstacles' entries and everything else restored; per launch, everything it could have touched comes back as numpy.  The batch is the rows of
    `inp`'s arrays (feature_kernel_cases.inputs: twelve; feature_kernel_cases.embed: a batch the scheduler deals).  alpha: an explicit slack
    schedule (rows, N + 1), one more banded device array the handle reads in place (set_slack_schedule's device form).  scheduling: the handle's
    instance scheduling.  prime: in front of every measured launch one plain solve of the same batch through the fused entry without a step flag,
    `iters` wired -- it exists so that the measured launch has an order -- behind which everything is restored; `order` of the result is the
    permutation then in effect (None: the natural order)"""
    from mpc_gpu import _lib, pack_instance_bounds, pack_obstacle_mask
    B = inp["x0"].shape[0]
    N, no, level = inp["N"], inp["no"], inp["level"]
    dev = torch.device("cuda:0")
    q = torch.cuda.current_stream().cuda_stream
    words = pack_obstacle_mask(inp["mask"]).view(np.int32)
    out = []
    with make(mpc_gpu, N, no, B, scheduling=scheduling) as s:
        fk.configure(s, case)
        W0, We0, r0 = cfg_values(s)
        g0 = inp["groups"][0]
        assert float(s.cfg.thr0) == inp["thr0"] and np.array_equal(W0, g0["W"]) and np.array_equal(We0, g0["We"]) and (g0["r_safe"] == r0).all()
        table = pack_instance_bounds(s.cfg, B, **inp["bounds"])
        bd = Banded(torch, dev)
        put = lambda d, a: d.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        up = lambda a, mk: put(mk(*a.shape), a)
        dx0, dg, do, dn = up(inp["x0"], bd.f64), up(inp["goal"], bd.f64), up(inp["obst"], bd.f64), up(inp["noise"], bd.f64)
        X, U = bd.f64(B, N + 1, 5), bd.f64(B, N, 2)
        u0, cost, margin = bd.f64(B, 2), bd.f64(B), bd.f64(B)
        status, iters, steps, flags = bd.i32(B), bd.i32(B), bd.i32(B), bd.i32(B)
        iacc, sacc = bd.i32(B), bd.i32(B)
        feat = dict(yref=up(inp["yref"], bd.f64), offset=up(inp["offset"], bd.i32))
        s.set_reference(feat["yref"], feat["offset"])
        if level >= 2:
            feat.update(W=up(inp["W"], bd.f64), We=up(inp["We"], bd.f64), r_safe=up(inp["r_safe"], bd.f64))
            s.set_instance_params(W=feat["W"], We=feat["We"], r_safe=feat["r_safe"])
        if level >= 3:
            feat["words"] = up(words, bd.i32)
            s.set_obstacle_mask(feat["words"])
        if level >= 4:
            feat["table"] = up(table, bd.f64)
            s.set_instance_bounds_dev(feat["table"])
        if alpha is not None:
            feat["alpha"] = up(alpha, bd.f64)
            s.set_slack_schedule(feat["alpha"])
        torch.cuda.current_stream().synchronize()
        name = s.kernel_name(B)
        assert name == case["name"], (name, case["name"])             # before anything is launched
        s.set_accumulators(iacc, sacc)
        uploaded = dict(goal=(dg, inp["goal"]), noise=(dn, inp["noise"]), yref=(feat["yref"], inp["yref"]))
        if level >= 2:
            uploaded.update(W=(feat["W"], inp["W"]), We=(feat["We"], inp["We"]), r_safe=(feat["r_safe"], inp["r_safe"]))
        if level >= 3:
            uploaded["mask words"] = (feat["words"], words)
        if level >= 4:
            uploaded["bounds table"] = (feat["table"], table)
        if alpha is not None:
            uploaded["slack schedule"] = (feat["alpha"], alpha)
        c = lambda a: a.cpu().numpy().copy()
        fl = _lib.STEP_SHIFT | _lib.STEP_PLANT | _lib.STEP_OBSTACLES | _lib.STEP_METRICS | _lib.STEP_RESET_ON_FAIL | _lib.STEP_ADVANCE_REF
        def restore(obst):
            put(dx0, inp["x0"]); put(do, obst); put(flags, inp["ep_flags"]); put(feat["offset"], inp["offset"])
            u0.fill_(-5.0); cost.fill_(-5.0); margin.fill_(float("inf")); status.fill_(-9); iters.fill_(-9); steps.fill_(100); iacc.fill_(1000); sacc.fill_(0)
            s.reset_guess_dev(B, dx0, X, U, stream=q)
            torch.cuda.current_stream().synchronize()

        for nan_absent in (False, True) if nan_absent_too else (False,):
            obst = inp["obst"].copy()
            if nan_absent:
                obst[~inp["mask"]] = np.nan
            restore(obst)
            if prime:
                s.closed_loop_step_dev(B, dx0, do, dg, X, U, u0, cost, status, iters, flags=0, ep_flags=flags, stream=q)
                restore(obst)
            order = s.instance_order(B) if prime else None      # (still there behind the restore: nothing but the scheduling switch or another batch size clears it)
            X0, U0 = c(X), c(U)
            s.closed_loop_step_dev(B, dx0, do, dg, X, U, u0, cost, status, iters, dn, RANDOMNESS, VMAX, flags=fl, min_margin=margin, ep_flags=flags, ep_steps=steps, stream=q)
            torch.cuda.current_stream().synchronize()
            out.append(dict(name=name, order=order, X0=X0, U0=U0, obst_in=obst, x0=c(dx0), obst=c(do), X=c(X), U=c(U), u0=c(u0), cost=c(cost), margin=c(margin),
                            status=c(status), iters=c(iters), flags=c(flags), steps=c(steps), iacc=c(iacc), sacc=c(sacc), offset=c(feat["offset"]),
                            intact=bd.intact(), written=[k for k, (d, h) in uploaded.items() if not np.array_equal(c(d), h)]))
        s.set_accumulators(None, None)
    return out


OUTPUTS = ("x0", "obst", "X", "U", "u0", "cost", "margin", "status", "iters", "flags", "steps", "iacc", "sacc", "offset")


def _placement(inp, r, why):
    N = inp["N"]
    stepped = inp["ep_flags"] == 0
    idle = ~stepped
    if not r["intact"]: why.append("a guard band was written")
    if r["written"]: why.append(f"written by the launch: {r['written']}")
    if not np.array_equal(r["offset"], inp["offset"] + stepped): why.append(f"reference offsets {r['offset'].tolist()} from {inp['offset'].tolist()}")
    if not np.isin(r["status"][stepped], (0, 2, 4)).all(): why.append(f"status values {r['status'].tolist()}")
    if not np.array_equal(r["iacc"][stepped], 1000 + r["iters"][stepped]): why.append(f"iteration accumulator {(r['iacc'] - 1000).tolist()} vs {r['iters'].tolist()}")
    if not np.array_equal(r["sacc"][stepped], ((r["status"] == 4) + 65536 * (r["status"] == 2))[stepped]): why.append("status accumulator")
    if not np.array_equal(r["steps"][stepped], (100 + ((r["flags"] & 1) == 0))[stepped]): why.append(f"step counters {r['steps'].tolist()}")
    if (r["flags"][0] & 1) != 1: why.append("instance 0 did not reach its goal")
    if not np.array_equal(r["X"][stepped, N], r["X"][stepped, N - 1]): why.append("the shift did not keep the terminal state")
    if not (r["U"][stepped, N - 1] == 0.0).all(): why.append("the shift did not clear the last input")
    # the idle instance: nothing of it is touched (accumulators included: the solve tail stores nothing for it)
    init = dict(x0=inp["x0"], obst=r["obst_in"], X=r["X0"], U=r["U0"], u0=np.full((B, 2), -5.0), cost=np.full(B, -5.0), margin=np.full(B, np.inf),
                status=np.full(B, -9), iters=np.full(B, -9), flags=inp["ep_flags"], steps=np.full(B, 100), iacc=np.full(B, 1000), sacc=np.zeros(B, int),
                offset=inp["offset"])
    for k, v in init.items():
        if not np.array_equal(r[k][idle], v[idle], equal_nan=(k == "obst")): why.append(f"the idle instance's {k} was written")


def _against_oracle(orc, inp, r, why, rep, alpha=None):
    """the solve, group by group, from the reset guess: the iterate un-shifted (stage 0 is the state the solve started from, u*[0] the applied input).
    alpha: the explicit slack schedule the launch ran with; a group's instances keep their own rows (an absent obstacle has no row whatever the weight)"""
    N = inp["N"]
    Xn = np.concatenate([inp["x0"][:, None, :], r["X"][:, :N]], axis=1)
    Un = np.concatenate([r["u0"][:, None, :], r["U"][:, :N - 1]], axis=1)
    judged = 0
    for k in range(fk.GROUPS):
        idx, cfg, Pk, radii = fk.group_problem(orc, inp, k)
        live = inp["ep_flags"][idx] == 0
        idx, Pk = idx[live], np.ascontiguousarray(Pk[live])
        gb = {name: r[name][idx] for name in ("u0", "cost", "status", "iters")}
        ak = None if alpha is None else np.ascontiguousarray(alpha[idx])
        try:
            with orc.obstacle_radii(radii):      # the oracle's solve, its trace and the exported QP of an adjudication all see the group's radii
                o = oracle_reference(orc, cfg, inp["x0"][idx], Pk, inp["goal"][idx], r["X0"][idx], r["U0"][idx], alpha=ak)
                n = judge_against_oracle(orc, cfg, inp["x0"][idx], Pk, inp["goal"][idx], r["X0"][idx], r["U0"][idx], gb, Xn[idx], Un[idx], o, alpha=ak)
        except AssertionError as e:
            why.append(f"group {k} against the oracle: {str(e)[:400]}")
            continue
        judged += n["judged_by_qp"]
        rep["converged"] += n["converged"]; rep["adjudicated"] += n["judged_by_qp"]; rep["status_borderline"] += n["status_borderline"]
        rep["worst_gpu_oracle"] = max(rep["worst_gpu_oracle"], n["worst_d_gpu_oracle"]); rep["worst_gpu_exact"] = max(rep["worst_gpu_exact"], n["worst_d_gpu_exact"])
    if judged > allowed_adjudications(orc.config(N, inp["no"], 0.1 * N), B):       # the project's bound holds over the batch, not per group
        why.append(f"{judged} instances adjudicated over the batch")


def _moved(orc, inp, obst):
    """the obstacle states after the step: the oracle's obstacle_step with the same noise for every obstacle of an instance that stepped, absent ones too"""
    N, no = inp["N"], inp["no"]
    cfg = orc.config(N, no, 0.1 * N)
    ob = obst.copy()
    for b in np.nonzero(inp["ep_flags"] == 0)[0]:
        for j in range(no):
            ob[b, j] = orc.obstacle_step(cfg, obst[b, j], 0.1 * N / N, inp["noise"][b, j], RANDOMNESS, VMAX)
    return ob


def _bookkeeping(orc, inp, r, why):
    N, no, level = inp["N"], inp["no"], inp["level"]
    dt = 0.1 * N / N
    stepped = inp["ep_flags"] == 0
    cfg = orc.config(N, no, 0.1 * N)
    x, ob = inp["x0"].copy(), _moved(orc, inp, inp["obst"])
    for b in np.nonzero(stepped)[0]:
        x[b] = orc.dynamics(inp["x0"][b], r["u0"][b], dt)[0]
    if np.abs(r["x0"] - x).max() > 1e-6: why.append(f"plant step differs by {np.abs(r['x0'] - x).max():.2e}")
    if not np.array_equal(r["obst"], ob): why.append("obstacle motion")
    r_hit = inp["r_safe"] - 1.2 if level >= 2 else np.full((B, no), 1.2)
    mm = np.full(B, np.inf); fl = inp["ep_flags"].copy(); ns = np.full(B, 100, np.int32)
    step_bookkeeping(x, ob, inp["goal"], inp["mask"], r_hit, [float(v) for v in cfg.arena], stepped, mm, fl, ns)
    if not np.array_equal(np.isfinite(r["margin"]), np.isfinite(mm)) or np.abs(r["margin"] - mm)[np.isfinite(mm)].max(initial=0.0) > 1e-6:
        why.append(f"min_margin {r['margin'].tolist()} vs {mm.tolist()}")
    hit_bit = np.where(np.abs(mm) > 1e-9, 4, 0)      # (a margin within 1e-9 of zero: the hit flag alone is not compared)
    if not np.array_equal(r["flags"] & (3 | hit_bit), fl & (3 | hit_bit)): why.append(f"episode flags {r['flags'].tolist()} vs {fl.tolist()}")
    if not np.array_equal(r["steps"], ns): why.append(f"step counters {r['steps'].tolist()} vs {ns.tolist()}")


def _nan_launch_is_the_first(inp, r, again, why, nan_ok=()):
    """levels 3 and 4: the launch with NaN in the absent obstacles' entries (`again`) against the one without (`r`), over every row of the batch.
    nan_ok: outputs in which a NaN of the first launch (a failed filler's) is one of the second"""
    absent = ~inp["mask"]
    assert absent.any()
    for k in OUTPUTS:
        if k == "obst":
            # the absent obstacles move too.  Their positions stay NaN.  Their velocities go through the noise clamp fmin(fmax(v, -vmax), vmax),
            # and IEEE fmax / fmin return the other operand of a NaN: fmax(NaN, -vmax) = -vmax, fmin(-vmax, vmax) = -vmax; the wall test then
            # compares NaN, takes the plain arm and keeps the velocity.  So an absent row of an instance that stepped is exactly
            # (NaN, NaN, -vmax, -vmax); the idle instance's rows are untouched, NaN throughout.
            want = np.full(again[k].shape, np.nan)
            want[..., 2:] = -VMAX
            want[inp["ep_flags"] != 0] = np.nan
            same = np.array_equal(again[k][~absent], r[k][~absent]) and np.array_equal(again[k][absent], want[absent], equal_nan=True)
            if not same: why.append(f"absent rows after the step: {again[k][absent].tolist()[:4]}")
        else:
            same = np.array_equal(again[k], r[k], equal_nan=k in nan_ok)
        if not same: why.append(f"NaN in the absent obstacles' entries changed {k}")
    if not again["intact"] or again["written"]: why.append(f"second launch: bands {again['intact']}, written {again['written']}")


def _body(mg, family, level, schedule_of=None):
    """schedule_of(orc, case): (inputs, alpha) -- the case's inputs in the schedule sweep's world and the explicit slack schedule (B, N + 1) layered
    on top of them (None: the case's own inputs, the built-in schedule)"""
    import torch
    mpc_gpu, orc = mg
    cases = fk.cases_of(family, level)
    bad, ran = [], []
    for case in cases:
        inp, alpha = (fk.inputs(orc, case), None) if schedule_of is None else schedule_of(orc, case)
        with torch.cuda.stream(torch.cuda.Stream()):      # a stream of its own per kernel
            r, again = (_launches(mpc_gpu, torch, case, inp, level >= 3, alpha) + [None])[:2]
        ran.append(r["name"])
        why = []
        rep = dict(converged=0, adjudicated=0, status_borderline=0, worst_gpu_oracle=0.0, worst_gpu_exact=0.0)
        _placement(inp, r, why)
        _against_oracle(orc, inp, r, why, rep, alpha)
        _bookkeeping(orc, inp, r, why)
        if again is not None:
            _nan_launch_is_the_first(inp, r, again, why)
        print(f"{'FEATURE-KERNEL' if alpha is None else 'SLACK-SCHEDULE level ' + str(level)} {r['name']} N {case['N']} n_obst {case['no']}: converged {rep['converged']} of {B - 1} worst_gpu_oracle {rep['worst_gpu_oracle']:.3e} "
              f"adjudicated {rep['adjudicated']} worst_gpu_exact {rep['worst_gpu_exact']:.3e} status_borderline {rep['status_borderline']} "
              f"status {r['status'].tolist()} {'FAILED: ' + '; '.join(why) if why else 'ok'}")
        if why:
            bad.append((case["name"], why))
    assert not bad, bad
    assert sorted(ran) == sorted(c["name"] for c in cases), ran      # nothing refused, nothing skipped


@pytest.mark.parametrize("level", fk.LEVELS)
@pytest.mark.parametrize("family", fk.FAMILIES)
def test_every_feature_instantiation_in_guard_bands_against_the_oracle(mg, family, level):
    on_own_stream(_body, mg, family, level)


def _schedule_of(world):
    def of(orc, case):
        import slack_schedule_cases as ss
        prob = ss.feature_problem(orc, case, world)
        return prob["inp"], prob["alpha"]
    return of


@pytest.mark.parametrize("world", ("crowded", "own"))
@pytest.mark.parametrize("level", fk.LEVELS)
@pytest.mark.parametrize("family", fk.FAMILIES)
def test_every_feature_instantiation_with_an_explicit_slack_schedule(mg, family, level, world):
    """the same sweep with slack_schedule_cases.schedule layered on top of every case's inputs: rows on the terminal stage,
    holes inside the horizon, a row per instance -- given as a banded device array, which the launch must leave as it was.  world "own": the case's
    own inputs as they are; "crowded": their obstacles aimed at the robots (slack_schedule_cases.crowded), where test_slack_schedule_host.py shows
    that every property of the schedule is felt by three instances or more"""
    on_own_stream(_body, mg, family, level, _schedule_of(world))
