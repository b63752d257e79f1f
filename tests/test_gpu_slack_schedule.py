"""An explicit slack schedule (mpc_set_slack_schedule / _dev) on EVERY solve kernel, against the oracle given the same schedule.

Every kernel reads the schedule the same way -- alpha[inst][stage], the terminal stage's weight unscaled, rows where the weight is positive -- and until
this file one instantiation of about 140 had run with one.  The schedule is slack_schedule_cases.schedule: rows on the terminal stage (which the built-in
schedule never has), holes inside the horizon, a row per instance, an instance without rows, one with terminal rows alone, one with the built-in values;
test_slack_schedule_host.py holds, on the oracle alone, that each of these is felt in every problem run here.
  1. level 0: every name kernel_configs.configs enumerates, a cold and a warm solve_dev of 37 instances in guard bands (here);
  2. levels 1 to 4: test_gpu_every_feature_kernel.py's second parametrisation;
  3. level 5: three SQP iterations in one launch against three launches, bit for bit, and against the oracle's three-fold sequence;
  4. around the read: the device form, packing with instance scheduling, the fused step, the config switches, the validation.
The tolerances are helpers.judge_against_oracle's (1e-6 on X, 8e-6 on u, cost to 1e-8, adjudications within allowed_adjudications, settled against the
exact solution of the QP exported WITH the instance's schedule)."""
import numpy as np
import pytest

import slack_schedule_cases as ss
import sqp_cases as sc
from feature_loop import Banded, assert_same, make, mg, on_own_stream, smallest_scheduled_batch
from helpers import fused_step_is_the_separate_calls, judge_against_oracle, oracle_reference
from kernel_configs import apply, configs

pytestmark = pytest.mark.gpu
INF = float("inf")


def _c(a):
    return a.cpu().numpy().copy()


def _solves(mpc_gpu, torch, prob, B, configure, name, launches=2, sqp=None, start=None, cfg_kw=None):
    """`launches` solve_dev of the problem's first B instances on a fresh handle, the first from the reset guess (or from `start` = (X, U)), every
    later one from the result; explicit P, the schedule through the host setter, every device array in a guard band.  The kernel name is asserted
    before the first launch.  Per launch: the iterate it started from and everything it wrote."""
    N, no = prob["N"], prob["no"]
    dev = torch.device("cuda:0")
    q = torch.cuda.current_stream().cuda_stream
    P = prob["inp"]["P"] if "inp" in prob else prob["groups"][0]["P"]
    out = []
    with make(mpc_gpu, N, no, B, **(cfg_kw or {})) as s:
        configure(s)
        if sqp is not None:
            s.set_sqp(*sqp)
        s.set_slack_schedule(prob["alpha"][:B])
        got = s.kernel_name(B, lookahead=False)
        assert got == name, (got, name)                                 # before anything is launched
        bd = Banded(torch, dev)
        put = lambda d, a: d.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        up = lambda a: put(bd.f64(*a.shape), a)
        ins = dict(x0=prob["x0"][:B], P=P[:B], goal=prob["goal"][:B])
        dx0, dP, dg = up(ins["x0"]), up(ins["P"]), up(ins["goal"])
        X, U = bd.f64(B, N + 1, 5), bd.f64(B, N, 2)
        u0, cost = bd.f64(B, 2), bd.f64(B)
        status, iters, nsqp = bd.i32(B), bd.i32(B), bd.i32(B)
        if sqp is not None:
            s.set_sqp_iters_out(nsqp)
        if start is None:
            s.reset_guess_dev(B, dx0, X, U, stream=q)
        else:
            put(X, start[0]); put(U, start[1])
        for _ in range(launches):
            u0.fill_(-5.0); cost.fill_(-5.0); status.fill_(-9); iters.fill_(-9); nsqp.fill_(-77)
            torch.cuda.current_stream().synchronize()
            X0, U0 = _c(X), _c(U)
            s.solve_dev(B, dx0, dP, dg, X, U, u0, cost, status, iters, stream=q)
            torch.cuda.current_stream().synchronize()
            out.append(dict(X0=X0, U0=U0, X=_c(X), U=_c(U), u0=_c(u0), cost=_c(cost), status=_c(status), iters=_c(iters), sqp_iters=_c(nsqp), intact=bd.intact(),
                            inputs_kept=all(np.array_equal(_c(d), ins[k], equal_nan=True) for d, k in ((dx0, "x0"), (dP, "P"), (dg, "goal")))))
    return out


def _judge(orc, prob, idx, r, rep):
    """one launch over the instances idx of a one-group problem against the oracle given the same rows of the schedule"""
    (g,) = prob["groups"]
    idx = np.asarray(idx)
    cfg, alpha = g["cfg"], np.ascontiguousarray(prob["alpha"][idx])
    x0, P, goal = prob["x0"][idx], np.ascontiguousarray(g["P"][idx]), prob["goal"][idx]
    o = oracle_reference(orc, cfg, x0, P, goal, r["X0"][idx], r["U0"][idx], alpha=alpha)
    gb = {k: r[k][idx] for k in ("u0", "cost", "status", "iters")}
    n = judge_against_oracle(orc, cfg, x0, P, goal, r["X0"][idx], r["U0"][idx], gb, r["X"][idx], r["U"][idx], o, alpha=alpha)
    rep["converged"] += n["converged"]; rep["adjudicated"] += n["judged_by_qp"]; rep["status_borderline"] += n["status_borderline"]
    rep["worst_gpu_oracle"] = max(rep["worst_gpu_oracle"], n["worst_d_gpu_oracle"]); rep["worst_gpu_exact"] = max(rep["worst_gpu_exact"], n["worst_d_gpu_exact"])
    return n


def _rep():
    return dict(converged=0, adjudicated=0, status_borderline=0, worst_gpu_oracle=0.0, worst_gpu_exact=0.0)


def _line(rep):
    return (f"converged {rep['converged']} worst_gpu_oracle {rep['worst_gpu_oracle']:.3e} adjudicated {rep['adjudicated']} worst_gpu_exact {rep['worst_gpu_exact']:.3e} "
            f"status_borderline {rep['status_borderline']}")


# ---------------------------------------------------------------------------------------------------------------- 1. level 0
def _every_level0_kernel(mg):
    import torch
    mpc_gpu, orc = mg
    B = ss.LEVEL0_B
    cfgs = configs(mpc_gpu, batch=B, lookahead=False)
    names = [c[3] for c in cfgs]
    assert len(cfgs) >= 40, names
    bad, ran, refused = [], [], []
    for N, no, ov, name in cfgs:
        prob = ss.level0_problem(orc, N, no)
        try:
            with torch.cuda.stream(torch.cuda.Stream()):      # a stream of its own per kernel
                cold, warm = _solves(mpc_gpu, torch, prob, B, lambda s: apply(s, ov), name)
        except mpc_gpu.MpcError as e:
            assert "no kernel variant" in str(e), (name, str(e))      # a combination of overrides the dispatcher refuses (it names a kernel that is not instantiated)
            refused.append(name)
            continue
        ran.append(name)
        why, rep = [], _rep()
        for what, r in (("cold", cold), ("warm", warm)):
            if not (r["intact"] and r["inputs_kept"]): why.append(f"{what}: a guard band or an input array was written")
            if not np.isin(r["status"], (0, 2, 4)).all(): why.append(f"{what}: status values {r['status'].tolist()}")
            try:
                _judge(orc, prob, np.arange(B), r, rep)
            except AssertionError as e:
                why.append(f"{what} against the oracle: {str(e)[:400]}")
        if not np.array_equal(warm["X0"], cold["X"]): why.append("the warm solve did not start from the cold one's result")
        print(f"SLACK-SCHEDULE level 0 {name} N {N} n_obst {no}: {_line(rep)} of {2 * B} {'FAILED: ' + '; '.join(why) if why else 'ok'}")
        if why:
            bad.append((name, why))
    print(f"SLACK-SCHEDULE level 0: ran {len(ran)}, refused by the dispatcher {refused}")
    assert not bad, bad
    assert len(set(ran)) >= 40 and any("rti_solve_kernel<3, 32, 2, false>" in n for n in ran), (sorted(set(ran)), refused)
    assert sorted(ran + refused) == sorted(names)              # every enumerated name ran or was refused by the dispatcher


def test_every_level_zero_kernel_cold_and_warm_against_the_oracle(mg):
    on_own_stream(_every_level0_kernel, mg)


# ---------------------------------------------------------------------------------------------------------------- 3. level 5
def _three_in_one_launch(mg, cid, world):
    import torch
    mpc_gpu, orc = mg
    c = sc.case(cid)
    prob = ss.sqp_problem(orc, c, world)
    B = sc.B
    nothing = lambda s: None
    (a,) = _solves(mpc_gpu, torch, prob, B, nothing, c["name"], launches=1, sqp=(3, 0.0), start=(prob["X0"], prob["U0"]))
    assert a["intact"] and a["inputs_kept"]
    # three launches of one iteration each on the same kernel (set_sqp(2, inf) stops behind its first iteration); an instance whose solve failed stops
    X, U = prob["X0"].copy(), prob["U0"].copy()
    live = np.ones(B, bool)
    last = dict(u0=np.zeros((B, 2)), cost=np.zeros(B), status=np.zeros(B, np.int32))
    it_sum, count = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for k in range(1, 4):
        (r,) = _solves(mpc_gpu, torch, prob, B, nothing, c["name"], launches=1, sqp=(2, INF), start=(X, U))
        assert r["intact"] and r["inputs_kept"] and (r["sqp_iters"] == 1).all()
        for b in np.nonzero(live)[0]:
            X[b], U[b] = r["X"][b], r["U"][b]
            for key in last:
                last[key][b] = r[key][b]
            it_sum[b] += r["iters"][b]; count[b] = k
            if r["status"][b] == 4:
                live[b] = False
    assert np.array_equal(a["sqp_iters"], count), (a["sqp_iters"], count)
    for key, want in (("X", X), ("U", U), ("u0", last["u0"]), ("cost", last["cost"]), ("status", last["status"]), ("iters", it_sum)):
        assert np.array_equal(a[key], want, equal_nan=(key == "cost")), key
    # ... and the oracle's three-fold sequence with the same schedule
    o = sc.oracle_sequence(orc, c, step_tol=0.0, max_iter=3, alpha=prob["alpha"], P=prob["inp"]["P"])
    fin = sc.finite_instances()
    dX = np.abs(a["X"][fin] - o["X"][fin]).max(axis=(1, 2)); dU = np.abs(a["U"][fin] - o["U"][fin]).max(axis=(1, 2))
    du0 = np.abs(a["u0"][fin] - o["u0"][fin]).max(axis=1)
    print(f"SLACK-SCHEDULE level 5 {world} {cid} {c['name']}: converged {int((a['status'][fin] == 0).sum())} of {len(fin)} worst |dX| {dX.max():.3e} |dU| {dU.max():.3e} "
          f"|du0| {du0.max():.3e} adjudicated 0; iterations {a['sqp_iters'].tolist()}; interior-point iterations {a['iters'].tolist()} vs {o['iters'].tolist()}")
    assert np.array_equal(a["status"], o["status"]), (a["status"], o["status"])
    assert np.array_equal(a["sqp_iters"], o["sqp_iters"]) and (a["sqp_iters"][fin] == 3).all(), (a["sqp_iters"], o["sqp_iters"])
    assert (dX <= 1e-6).all(), dX
    assert (dU <= 8e-6).all() and (du0 <= 8e-6).all(), (dU, du0)
    assert np.allclose(a["cost"][fin], o["cost"][fin], rtol=1e-8, atol=0.0)
    n = sc.NAN_INSTANCE                     # the NaN instance is as before: status 4 at once, one iteration, the iterate untouched
    assert a["status"][n] == 4 and a["sqp_iters"][n] == 1
    assert np.array_equal(a["X"][n], prob["X0"][n]) and np.array_equal(a["U"][n], prob["U0"][n])


@pytest.mark.parametrize("world", ss.WORLDS)
@pytest.mark.parametrize("cid", sc.IDS)
def test_three_sqp_iterations_in_one_launch_with_a_schedule(mg, cid, world):
    on_own_stream(_three_in_one_launch, mg, cid, world)


# ---------------------------------------------------------------------------------------------------------------- 4. around the read
FAMILY_KERNEL = {"split": "rti_split_kernel<3, 3,", "one": "rti_solve_kernel<3, 64,", "wide": "rti_wide_kernel<20, 2,"}


def _run(s, prob, B, steps=2):
    """reset guess, `steps` solves with explicit P, everything a caller sees (feature_loop.run with explicit P)"""
    P = prob["groups"][0]["P"]
    s.reset_guess(prob["x0"][:B])
    outs = []
    for _ in range(steps):
        o = s.solve(prob["x0"][:B], P[:B], prob["goal"][:B])
        X, U = s.get_traj(B)
        outs.append((X, U, o["u0"], o["cost"], o["status"], o["iters"]))
    return outs


def _device_form(mg, family):
    import torch
    mpc_gpu, orc = mg
    prob = ss.around_problem(orc, family)
    N, no, B = prob["N"], prob["no"], prob["B"]
    MB = B + 4                                  # max_batch: the device array has rows the solve does not read
    alpha, other = prob["alpha"], ss.next_row(prob["alpha"])
    dev = torch.device("cuda:0")

    def fresh(a):
        with make(mpc_gpu, N, no, MB) as s:
            assert s.kernel_name(B, lookahead=False).startswith(FAMILY_KERNEL[family]), s.kernel_name(B, lookahead=False)
            if a is not None:
                s.set_slack_schedule(a)
            return _run(s, prob, B)

    host, host_other, builtin = fresh(alpha), fresh(other), fresh(None)
    assert any((o[4] == 0).all() for o in host)
    with make(mpc_gpu, N, no, MB) as s:
        bd = Banded(torch, dev)
        d = bd.f64(MB, N + 1, init=7.0)         # (the rows behind the batch: finite decoys first)
        d[:B].copy_(torch.from_numpy(alpha).to(dev))
        torch.cuda.synchronize()
        s.set_slack_schedule(d)
        assert_same(_run(s, prob, B), host)
        d[B:] = float("nan")                    # a torch op: rows >= batch are never read
        torch.cuda.synchronize()
        assert_same(_run(s, prob, B), host)
        d[:B].copy_(torch.from_numpy(other).to(dev))      # the live rows rewritten in place, no library call
        torch.cuda.synchronize()
        assert_same(_run(s, prob, B), host_other)
        assert bd.intact() and np.array_equal(_c(d[:B]), other) and np.isnan(_c(d[B:])).all()
        s.set_slack_schedule(None)              # NULL: the built-in schedule again
        assert_same(_run(s, prob, B), builtin)
    differ = lambda a, b: int((np.abs(a[0][0] - b[0][0]).max(axis=(1, 2)) > ss.MOVED).sum())
    assert differ(host, host_other) >= ss.MIN_MOVED and differ(host, builtin) >= ss.MIN_MOVED


@pytest.mark.parametrize("family", list(ss.FAMILY_SHAPES))
def test_the_device_form_is_the_host_form(mg, family):
    on_own_stream(_device_form, mg, family)


def _packed(G):
    def configure(s):
        s.set_lanes_per_stage(1); s.set_lanes_per_instance(G)
    return configure


def _packed_and_scheduled(mg, G):
    mpc_gpu, orc = mg
    pool = ss.packed_problem(orc)
    N, no = pool["N"], pool["no"]
    P = pool["groups"][0]["P"]
    B = smallest_scheduled_batch(mpc_gpu, N, no, configure=_packed(G), key=("packed", G), limit=ss.PACKED_POOL)      # (raises if no batch of the pool is dealt)
    res = {}
    for on in (True, False):
        with mpc_gpu.BatchedMpc(N, no, 0.1 * N, max_batch=B) as s:
            s.set_lanes_per_stage(1); s.set_lanes_per_instance(G)
            s.set_instance_scheduling(on)
            s.set_slack_schedule(pool["alpha"][:B])
            name = s.kernel_name(B, lookahead=False)
            assert name.startswith(f"rti_solve_kernel<3, {G},"), name
            s.reset_guess(pool["x0"][:B])
            outs = []
            for k in range(3):
                X0, U0 = s.get_traj(B)
                o = s.solve(pool["x0"][:B], P[:B], pool["goal"][:B])
                X, U = s.get_traj(B)
                order = s.instance_order(B)
                assert (order is not None) == on, (k, on)       # from the first launch on: the batch is one the scheduler deals
                if on:
                    assert np.array_equal(np.sort(order), np.arange(B)) and not np.array_equal(order, np.arange(B))
                outs.append(dict(X0=X0, U0=U0, X=X, U=U, u0=o["u0"], cost=o["cost"], status=o["status"], iters=o["iters"]))
            res[on] = outs
    for a, b in zip(res[True], res[False]):
        for key in ("X", "U", "u0", "cost", "status", "iters"):
            assert np.array_equal(a[key], b[key]), key
    rep = _rep()
    for r in res[True]:
        _judge(orc, pool, np.arange(ss.PACKED_JUDGED), r, rep)
    print(f"SLACK-SCHEDULE packed {name} batch {B}: {_line(rep)} of {3 * ss.PACKED_JUDGED}")


@pytest.mark.parametrize("G", [16, 32])
def test_packed_instances_under_instance_scheduling(mg, G):
    on_own_stream(_packed_and_scheduled, mg, G)


def _fused(mg, family):
    from mpc_gpu import _lib
    mpc_gpu, orc = mg
    prob = ss.around_problem(orc, family)
    N, no, B = prob["N"], prob["no"], prob["B"]
    steps = 3
    noise = np.random.default_rng(78).standard_normal((steps, B, no, 2))

    def configure(s):
        s.set_slack_schedule(prob["alpha"])
        assert s.kernel_name(B).startswith(FAMILY_KERNEL[family]), s.kernel_name(B)

    flags = _lib.STEP_SHIFT | _lib.STEP_PLANT | _lib.STEP_OBSTACLES | _lib.STEP_RESET_ON_FAIL
    rec = fused_step_is_the_separate_calls(mpc_gpu, N, no, prob["x0"], prob["goal"], prob["obst"], noise, configure, flags, steps=steps)
    assert all((r["status"] == 0).any() for r in rec)
    # the first step against the oracle's own control step (the body of helpers.OracleLoop.step with the instance's row of the schedule)
    first, cfg = rec[0], prob["cfg"]
    Xn = np.concatenate([prob["x0"][:, None, :], first["X"][:, :N]], axis=1)          # the iterate un-shifted
    Un = np.concatenate([first["u0"][:, None, :], first["U"][:, :N - 1]], axis=1)
    r = dict(X0=prob["X0"], U0=prob["U0"], X=Xn, U=Un, u0=first["u0"], cost=first["cost"], status=first["status"], iters=first["iters"])
    rep = _rep()
    _judge(orc, prob, np.arange(B), r, rep)
    dt = cfg.Tf / N
    for b in range(B):          # what follows the solve in the oracle's control step: plant step, obstacle motion (bit for bit), warm-start shift
        o = orc.rti_solve(cfg, prob["x0"][b], orc.predict_params(cfg, prob["obst"][b]), prob["goal"][b], prob["X0"][b], prob["U0"][b], alpha=prob["alpha"][b])
        assert np.array_equal(first["obst"][b], np.stack([orc.obstacle_step(cfg, prob["obst"][b, j], dt, noise[0, b, j]) for j in range(no)]))
        if o["status"] == 0 and first["status"][b] == 0:
            assert np.abs(first["x"][b] - orc.dynamics(prob["x0"][b], first["u0"][b], dt)[0]).max() <= 1e-9
            assert np.array_equal(first["X"][b, N], first["X"][b, N - 1]) and (first["U"][b, N - 1] == 0.0).all()
    print(f"SLACK-SCHEDULE fused {family} N {N} n_obst {no}: {_line(rep)} of {B}")


@pytest.mark.parametrize("family", list(ss.FAMILY_SHAPES))
def test_fused_step_with_a_schedule_is_the_separate_calls(mg, family):
    on_own_stream(_fused, mg, family)


def _switch(mg, kw, packed):
    import torch
    mpc_gpu, orc = mg
    prob = ss.level0_problem(orc, *ss.PACKED_SHAPE, B=ss.AROUND_B, cfg_kw=kw, tag="around") if packed else ss.around_problem(orc, "split", cfg_kw=kw)
    B = prob["B"]

    def configure(s):
        if packed:
            s.set_lanes_per_stage(1); s.set_lanes_per_instance(32)

    name = ("rti_solve_kernel<3, 32, 2, false>" if packed else "rti_split_kernel<3, 3, false, false, false>")
    cold, warm = _solves(mpc_gpu, torch, prob, B, configure, name, cfg_kw=kw)
    rep = _rep()
    for r in (cold, warm):
        assert r["intact"] and r["inputs_kept"]
        _judge(orc, prob, np.arange(B), r, rep)
    print(f"SLACK-SCHEDULE switch {kw} {name}: {_line(rep)} of {2 * B} status {cold['status'].tolist()}")
    assert (cold["status"] == 0).sum() >= 3
    if "soft_h" in kw:
        # hard rows at every stage >= 1 whatever the schedule, zeros included: the all-zero schedule gives the same iterate bit for bit
        zero = dict(prob, alpha=np.zeros_like(prob["alpha"]))
        cold0, _ = _solves(mpc_gpu, torch, zero, B, configure, name, cfg_kw=kw)
        for key in ("X", "U", "u0", "status", "iters"):
            assert np.array_equal(cold0[key], cold[key]), key
        assert (cold["status"] == 4).any()
    else:
        # weights unscaled at every stage: the same schedule under the default config is another problem
        scaled, _ = _solves(mpc_gpu, torch, prob, B, configure, name)
        assert (np.abs(scaled["X"] - cold["X"]).max(axis=(1, 2)) > ss.MOVED).sum() >= ss.MIN_MOVED


@pytest.mark.parametrize("packed", [False, True], ids=["split", "packed32"])
@pytest.mark.parametrize("kw", ss.SWITCHES, ids=["slack_scale_dt0", "soft_h0"])
def test_config_switches_with_a_schedule(mg, kw, packed):
    on_own_stream(_switch, mg, kw, packed)


def _validation(mg):
    from mpc_gpu import _lib
    from mpc_gpu.solver import _ptr
    mpc_gpu, orc = mg
    prob = ss.around_problem(orc, "split")
    N, no, B = prob["N"], prob["no"], prob["B"]
    MB = B + 4
    alpha = prob["alpha"]
    L = _lib.lib()
    with make(mpc_gpu, N, no, MB) as s:
        s.set_slack_schedule(alpha)
        want = _run(s, prob, B)
        bad = {}
        for what, v in (("NaN", np.nan), ("+inf", np.inf), ("negative", -1.0), ("above 1e300", 1e301)):
            a = alpha.copy(); a[B - 1, N] = v       # the last entry: everything in front of it is valid
            bad[what] = (B, a)
        bad["batch 0 with a pointer"] = (0, alpha)
        bad["batch > max_batch"] = (MB + 1, np.ones((MB + 1, N + 1)))
        for what, (n, a) in bad.items():
            a = np.ascontiguousarray(a, dtype=np.float64)
            assert L.mpc_set_slack_schedule(s._h, n, _ptr(a)) == _lib.MPC_ERR_ARG, what
            assert_same(_run(s, prob, B), want)     # the schedule that was in effect is still in effect
        with pytest.raises(mpc_gpu.MpcError):
            s.set_slack_schedule(-alpha)
        # a schedule uploaded for k instances refuses a larger solve, and serves a solve of k
        k = 5
        s.set_slack_schedule(alpha[:k])
        with pytest.raises(mpc_gpu.MpcError, match="covers fewer instances"):
            _run(s, prob, B)
        assert_same(_run(s, prob, k), want, rows_b=slice(0, k))
        s.set_slack_schedule(alpha)
        assert_same(_run(s, prob, B), want)
    with make(mpc_gpu, N, no, MB) as s:             # (and `want` is not the built-in schedule's result)
        assert (np.abs(_run(s, prob, B)[0][0] - want[0][0]).max(axis=(1, 2)) > ss.MOVED).sum() >= ss.MIN_MOVED


def test_a_refused_schedule_leaves_the_one_in_effect(mg):
    on_own_stream(_validation, mg)
