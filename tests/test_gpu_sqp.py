"""Several SQP iterations per solve launch (mpc_set_sqp, feature level 5) on the GPU.  The specification is one sentence -- the result of a launch is
that of the same sequence of single-iteration launches stopped by the same rule -- and the tests are that sentence:

  1. K iterations in one launch against K launches of one iteration ON THE SAME KERNEL (set_sqp(2, inf) always stops behind its first iteration), the
     stop rule applied by the host between them: bit for bit, every case of sqp_cases, the iteration counts in a guard band;
  2. the same launch against the oracle's K-fold sequence (sqp_cases.oracle_sequence) within helpers.judge_against_oracle's tolerances (1e-6 on X,
     8e-6 on u), statuses and iteration counts equal, no adjudication (test_sqp_host.py holds what makes that fair);
     and once more with the case's twelve instances embedded in a batch that the instance scheduler deals (sqp_cases.embedded: fillers with feature
     rows of their own), scheduling on against off bit for bit over the whole batch, the iteration counts included;
  3. one level-5 iteration against the level-4 solve of the same handle with every lower feature set (feature_kernel_cases.inputs at level 4), by
     feature_loop.assert_same;
  4. the fused control step with three iterations against the separate calls, the idle instance, the reference offset;
  5. off means off, the kernel names, the refusals and the argument validation."""
import numpy as np
import pytest

import feature_kernel_cases as fk
import sqp_cases as sc
from feature_loop import Banded, assert_same, level_of, make, mg, on_own_stream, run, smallest_scheduled_batch
from helpers import fused_step_is_the_separate_calls, random_batch

pytestmark = pytest.mark.gpu
B, K = sc.B, sc.K
INF = float("inf")


def _launch(mpc_gpu, torch, c, inp, max_iter, step_tol, X, U):
    """one solve_dev of the case's batch from the iterate (X, U) (numpy) on a fresh handle with set_sqp(max_iter, step_tol); every output in a guard band"""
    N, no = inp["N"], inp["no"]
    dev = torch.device("cuda:0")
    q = torch.cuda.current_stream().cuda_stream
    with make(mpc_gpu, N, no, B, **c.get("cfg", {})) as s:
        s.set_sqp(max_iter, step_tol)
        name = s.kernel_name(B, lookahead=False)
        assert name == c["name"], (name, c["name"])      # before anything is launched
        bd = Banded(torch, dev)
        put = lambda d, a: d.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        up = lambda a: put(bd.f64(*a.shape), a)
        dx0, dP, dg, dX, dU = up(inp["x0"]), up(inp["P"]), up(inp["goal"]), up(X), up(U)
        u0, cost = bd.f64(B, 2, init=-5.0), bd.f64(B, init=-5.0)
        status, iters, nsqp = bd.i32(B, init=-9), bd.i32(B, init=-9), bd.i32(B, init=-77)
        s.set_sqp_iters_out(nsqp)
        torch.cuda.current_stream().synchronize()
        s.solve_dev(B, dx0, dP, dg, dX, dU, u0, cost, status, iters, stream=q)
        torch.cuda.current_stream().synchronize()
        g = lambda a: a.cpu().numpy().copy()
        return dict(X=g(dX), U=g(dU), u0=g(u0), cost=g(cost), status=g(status), iters=g(iters), sqp_iters=g(nsqp), intact=bd.intact(),
                    inputs_kept=all(np.array_equal(g(d), h, equal_nan=True) for d, h in ((dx0, inp["x0"]), (dP, inp["P"]), (dg, inp["goal"]))))


_ONE_LAUNCH = {}


def _one_launch(mg, c):
    """the case's K iterations in ONE launch, from the cold guess; run once per case and shared (tests 1 and 2)"""
    import torch
    mpc_gpu, orc = mg
    if c["id"] not in _ONE_LAUNCH:
        inp = sc.inputs(orc, c)
        _ONE_LAUNCH[c["id"]] = _launch(mpc_gpu, torch, c, inp, K, c["step_tol"], inp["X0"], inp["U0"])
    return _ONE_LAUNCH[c["id"]]


def _k_in_one_launch_is_k_launches(mg, cid):
    import torch
    mpc_gpu, orc = mg
    c = sc.case(cid)
    inp = sc.inputs(orc, c)
    a = _one_launch(mg, c)
    # the host-driven form: one iteration per launch on the same instantiation, the stop rule between the launches
    X, U = inp["X0"].copy(), inp["U0"].copy()
    live = np.ones(B, bool)
    last = dict(u0=np.zeros((B, 2)), cost=np.zeros(B), status=np.zeros(B, np.int32))
    it_sum, count = np.zeros(B, np.int32), np.zeros(B, np.int32)
    history = np.full((B, K), -1, np.int32)      # the status of every iteration run
    for k in range(1, K + 1):
        r = _launch(mpc_gpu, torch, c, inp, 2, INF, X, U)
        assert r["intact"] and r["inputs_kept"]
        assert (r["sqp_iters"] == 1).all(), r["sqp_iters"]      # (step_tol = inf: every instance stops behind its first iteration)
        for b in np.nonzero(live)[0]:
            nrm = sc.step_norm(X[b], U[b], r["X"][b], r["U"][b])
            if r["status"][b] == 4:
                assert np.array_equal(r["X"][b], X[b]) and np.array_equal(r["U"][b], U[b])
            X[b], U[b] = r["X"][b], r["U"][b]
            for key in last:
                last[key][b] = r[key][b]
            it_sum[b] += r["iters"][b]; count[b] = k; history[b, k - 1] = r["status"][b]
            if r["status"][b] == 4 or nrm <= c["step_tol"]:
                live[b] = False
    print(f"SQP {cid} {c['name']}: iterations per instance {a['sqp_iters'].tolist()} (host loop {count.tolist()}), status {a['status'].tolist()}, "
          f"interior-point iterations {a['iters'].tolist()}")
    assert a["intact"] and a["inputs_kept"]
    assert np.array_equal(a["sqp_iters"], count), (a["sqp_iters"], count)
    for key, want in (("X", X), ("U", U), ("u0", last["u0"]), ("cost", last["cost"]), ("status", last["status"]), ("iters", it_sum)):
        assert np.array_equal(a[key], want, equal_nan=(key == "cost")), key
    # the instance with a NaN in x0: status 4 at once, one iteration, the iterate untouched
    n = sc.NAN_INSTANCE
    assert a["status"][n] == 4 and a["sqp_iters"][n] == 1
    assert np.array_equal(a["X"][n], inp["X0"][n]) and np.array_equal(a["U"][n], inp["U0"][n])
    fin = sc.finite_instances()
    if cid == sc.STATUS2["id"]:
        # an iteration that ends at the interior point's cap (status 2) applies its step and the loop goes on: some instance has a 2 in front of a final 0
        print(f"SQP {cid}: statuses per iteration {history[fin].tolist()}")
        assert ((history[fin, :-1] == 2).any(axis=1) & (a["status"][fin] == 0) & (count[fin] == K)).any(), history
        assert (history[fin] != 4).all()
    else:
        assert len(set(a["sqp_iters"][fin].tolist())) >= 3 and (a["status"][fin] == 0).all()


@pytest.mark.parametrize("cid", sc.IDS + [sc.STATUS2["id"]])
def test_k_iterations_in_one_launch_are_k_launches_bit_for_bit(mg, cid):
    on_own_stream(_k_in_one_launch_is_k_launches, mg, cid)


def _judge_against_the_sequence(a, o, c, tag):
    """one launch's rows of the case's twelve instances (a) against the oracle's K-fold sequence (o)"""
    fin = sc.finite_instances()
    dX = np.abs(a["X"][fin] - o["X"][fin]).max(axis=(1, 2)); dU = np.abs(a["U"][fin] - o["U"][fin]).max(axis=(1, 2))
    du0 = np.abs(a["u0"][fin] - o["u0"][fin]).max(axis=1)
    print(f"{tag} {c['id']} {c['name']}: worst |dX| {dX.max():.3e} |dU| {dU.max():.3e} |du0| {du0.max():.3e}; iterations {a['sqp_iters'].tolist()} "
          f"vs {o['sqp_iters'].tolist()}; interior-point iterations {a['iters'].tolist()} vs {o['iters'].tolist()}")
    assert np.array_equal(a["status"], o["status"]), (a["status"], o["status"])
    assert np.array_equal(a["sqp_iters"], o["sqp_iters"]), (a["sqp_iters"], o["sqp_iters"])
    assert (dX <= 1e-6).all(), dX          # (no adjudication: every instance is within the tolerance outright)
    assert (dU <= 8e-6).all() and (du0 <= 8e-6).all(), (dU, du0)
    assert np.allclose(a["cost"][fin], o["cost"][fin], rtol=1e-8, atol=1e-8)
    n = sc.NAN_INSTANCE
    assert np.array_equal(a["X"][n], o["X"][n]) and np.array_equal(a["U"][n], o["U"][n])


def _against_the_oracle(mg, cid):
    mpc_gpu, orc = mg
    c = sc.case(cid)
    _judge_against_the_sequence(_one_launch(mg, c), sc.oracle_sequence(orc, c), c, "SQP-ORACLE")


@pytest.mark.parametrize("cid", sc.IDS)
def test_one_launch_against_the_oracle_sequence(mg, cid):
    on_own_stream(_against_the_oracle, mg, cid)


# ---------------------------------------------------------------------------------------------------------------- 2b. the same launch in a batch the scheduler deals
SCHEDULED_OUT = ("X", "U", "u0", "cost", "status", "iters", "sqp_iters")


def _launch_embedded(mpc_gpu, torch, c, e, scheduling):
    """the case's K iterations in one solve_dev of the embedded batch (sqp_cases.embedded) from the cold guess, on a fresh handle that reads every
    per-instance table in its device form; in front of it a priming launch of the same batch -- so that the measured one has an order -- behind
    which the iterate and every output sentinel are restored.  Every array in a guard band"""
    from mpc_gpu import pack_instance_bounds, pack_obstacle_mask
    N, no, Bs = e["N"], e["no"], e["Bs"]
    dev = torch.device("cuda:0")
    q = torch.cuda.current_stream().cuda_stream
    with make(mpc_gpu, N, no, Bs, scheduling=scheduling, **c.get("cfg", {})) as s:
        s.set_sqp(K, c["step_tol"])
        bd = Banded(torch, dev)
        put = lambda d, a: d.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        up = lambda a, mk=bd.f64: put(mk(*a.shape), a)
        ins = dict(x0=e["x0"], P=e["P"], goal=e["goal"], yref=e["yref"], offset=e["offset"], W=e["W"], We=e["We"], r_safe=e["r_safe"],
                   words=pack_obstacle_mask(e["mask"]).view(np.int32), table=pack_instance_bounds(s.cfg, Bs, **e["bounds"]))
        d = {k: up(a, bd.i32 if a.dtype == np.int32 else bd.f64) for k, a in ins.items()}
        s.set_reference(d["yref"], d["offset"])
        s.set_instance_params(W=d["W"], We=d["We"], r_safe=d["r_safe"])
        s.set_obstacle_mask(d["words"])
        s.set_instance_bounds_dev(d["table"])
        name = s.kernel_name(Bs, lookahead=False)
        assert name == c["name"], (name, c["name"])      # before anything is launched
        dX, dU = bd.f64(Bs, N + 1, 5), bd.f64(Bs, N, 2)
        u0, cost = bd.f64(Bs, 2), bd.f64(Bs)
        status, iters, nsqp = bd.i32(Bs), bd.i32(Bs), bd.i32(Bs)
        s.set_sqp_iters_out(nsqp)

        def restore():
            put(dX, e["X0"]); put(dU, e["U0"])
            u0.fill_(-5.0); cost.fill_(-5.0); status.fill_(-9); iters.fill_(-9); nsqp.fill_(-77)
            torch.cuda.current_stream().synchronize()

        restore()
        s.solve_dev(Bs, d["x0"], d["P"], d["goal"], dX, dU, u0, cost, status, iters, stream=q)      # the priming launch
        restore()
        order = s.instance_order(Bs)
        s.solve_dev(Bs, d["x0"], d["P"], d["goal"], dX, dU, u0, cost, status, iters, stream=q)
        torch.cuda.current_stream().synchronize()
        g = lambda a: a.cpu().numpy().copy()
        return dict(X=g(dX), U=g(dU), u0=g(u0), cost=g(cost), status=g(status), iters=g(iters), sqp_iters=g(nsqp), order=order, intact=bd.intact(),
                    inputs_kept=all(np.array_equal(g(d[k]), ins[k], equal_nan=True) for k in ins))


def _scheduled(mg, cid):
    import torch
    from test_gpu_feature_scheduling import order_facts
    mpc_gpu, orc = mg
    c = sc.case(cid)
    Bs = smallest_scheduled_batch(mpc_gpu)
    pos = fk.positions(Bs)
    e = sc.embedded(orc, c, Bs, pos)
    runs = {}
    for on in (True, False):
        with torch.cuda.stream(torch.cuda.Stream()):
            runs[on] = _launch_embedded(mpc_gpu, torch, c, e, on)
    a, off = runs[True], runs[False]
    live = pos[sc.finite_instances()]
    why, moved, far = order_facts(a["order"], Bs, live)
    print(f"SQP scheduled {cid} {c['name']} Bs {Bs}: moved {moved} of {len(live)} farthest {far}; fillers with status 0 / 2 / 4 "
          f"{[int((a['status'][e['filler']] == v).sum()) for v in (0, 2, 4)]}, their iteration counts {np.bincount(a['sqp_iters'][e['filler']], minlength=K + 1).tolist()}")
    assert not why, why
    assert off["order"] is None
    for r in (a, off):
        assert r["intact"] and r["inputs_kept"]
    for k in SCHEDULED_OUT:      # all Bs rows, scheduling on against off
        assert np.array_equal(a[k], off[k], equal_nan=(k == "cost")), (k, np.nonzero((a[k] != off[k]).reshape(Bs, -1).any(axis=1))[0][:8])
    _judge_against_the_sequence({k: a[k][pos] for k in SCHEDULED_OUT}, sc.oracle_sequence(orc, c), c, "SQP-ORACLE scheduled")
    for n in (pos[sc.NAN_INSTANCE], e["nan_filler"]):      # a NaN in x0: status 4 at once, one iteration, the iterate untouched
        assert a["status"][n] == 4 and a["sqp_iters"][n] == 1
        assert np.array_equal(a["X"][n], e["X0"][n]) and np.array_equal(a["U"][n], e["U0"][n])
    assert np.isin(a["status"], (0, 2, 4)).all() and ((a["sqp_iters"] >= 1) & (a["sqp_iters"] <= K)).all()


@pytest.mark.parametrize("cid", sc.IDS)
def test_one_launch_in_a_scheduled_batch_against_the_oracle_sequence(mg, cid):
    on_own_stream(_scheduled, mg, cid)


def _one_iteration_is_the_level_four_solve(mg, family):
    mpc_gpu, orc = mg
    ran = []
    for case in fk.cases_of(family, 4):
        inp = fk.inputs(orc, case)
        with make(mpc_gpu, inp["N"], inp["no"], fk.B) as s:
            fk.configure(s, case)
            s.set_reference(inp["yref"], inp["offset"])
            s.set_instance_params(W=inp["W"], We=inp["We"], r_safe=inp["r_safe"])
            s.set_obstacle_mask(inp["mask"])
            s.set_instance_bounds(**inp["bounds"])
            assert s.kernel_name(fk.B) == case["name"]
            off = run(s, inp["x0"], inp["obst"], inp["goal"])
            s.set_sqp(2, INF)
            name = s.kernel_name(fk.B)
            assert level_of(name) == 5 and name == case["name"].replace(">", ", true>"), name
            on = run(s, inp["x0"], inp["obst"], inp["goal"])
            s.set_sqp(1, 0.0)
            assert s.kernel_name(fk.B) == case["name"]
        assert_same(on, off)
        assert any((o[4] == 0).any() for o in on)
        ran.append(name)
    assert len(ran) == len(set(ran)) == {"one": 3, "split": 6, "wide": 2}[family]


@pytest.mark.parametrize("family", fk.FAMILIES)
def test_one_level_five_iteration_is_the_level_four_solve(mg, family):
    on_own_stream(_one_iteration_is_the_level_four_solve, mg, family)


FUSED = ("split3-3", "wide-20")      # one stage-split case, one multi-wavefront case


def _fused_inputs(orc, c):
    inp = sc.inputs(orc, c)
    x0 = inp["x0"].copy()
    x0[sc.NAN_INSTANCE, 1] = 0.5      # (finite here: the NaN case of the fused step is test_gpu_solve_tail.py's)
    return inp, x0


def _fused_step_is_the_separate_calls(mg, cid):
    from mpc_gpu import _lib
    mpc_gpu, orc = mg
    c = sc.case(cid)
    inp, x0 = _fused_inputs(orc, c)
    steps = 3
    noise = np.random.default_rng(77).standard_normal((steps, B, inp["no"], 2))

    def configure(s):
        s.set_sqp(3, c["step_tol"])
        assert s.kernel_name(B) == c["name"]

    flags = _lib.STEP_SHIFT | _lib.STEP_PLANT | _lib.STEP_OBSTACLES
    rec = fused_step_is_the_separate_calls(mpc_gpu, inp["N"], inp["no"], x0, inp["goal"], inp["obst"], noise, configure, flags, steps=steps)
    assert all((r["status"] == 0).any() for r in rec)


@pytest.mark.parametrize("cid", FUSED)
def test_fused_step_with_three_iterations_is_the_separate_calls(mg, cid):
    on_own_stream(_fused_step_is_the_separate_calls, mg, cid)


def _fused_idle_and_reference(mg, cid):
    """three fused steps with the bookkeeping: the idle instance's words -- its iteration count among them -- are untouched, the reference offset moves
    by one per control step (not per iteration), and the counts lie in [1, 3]"""
    import torch
    from mpc_gpu import _lib
    mpc_gpu, orc = mg
    c = sc.case(cid)
    inp, x0 = _fused_inputs(orc, c)
    N, no = inp["N"], inp["no"]
    dev = torch.device("cuda:0")
    q = torch.cuda.current_stream().cuda_stream
    idle = sc.IDLE_INSTANCE
    yref = np.zeros((B, N + 8, 6)); yref[:, :, :2] = inp["goal"][:, None, :]
    with make(mpc_gpu, N, no, B) as s:
        s.set_sqp(3, c["step_tol"])
        bd = Banded(torch, dev)
        put = lambda d, a: d.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        up = lambda a, mk: put(mk(*a.shape), a)
        dx0, dg, do = up(x0, bd.f64), up(inp["goal"], bd.f64), up(inp["obst"], bd.f64)
        dy, doff = up(yref, bd.f64), bd.i32(B, init=2)
        X, U = bd.f64(B, N + 1, 5), bd.f64(B, N, 2)
        u0, cost, margin = bd.f64(B, 2, init=-5.0), bd.f64(B, init=-5.0), bd.f64(B, init=INF)
        status, iters, nsqp = bd.i32(B, init=-9), bd.i32(B, init=-9), bd.i32(B, init=-77)
        flags, steps = bd.i32(B), bd.i32(B, init=100)
        flags[idle] = 1
        s.set_reference(dy, doff)
        s.set_sqp_iters_out(nsqp)
        assert s.kernel_name(B) == c["name"]
        s.reset_guess_dev(B, dx0, X, U, stream=q)
        torch.cuda.current_stream().synchronize()
        g = lambda a: a.cpu().numpy().copy()
        X0, U0 = g(X), g(U)
        fl = _lib.STEP_SHIFT | _lib.STEP_PLANT | _lib.STEP_OBSTACLES | _lib.STEP_METRICS | _lib.STEP_RESET_ON_FAIL | _lib.STEP_ADVANCE_REF
        stepped = np.zeros(B, np.int32)
        for k in range(3):
            alive = (g(flags) & 1) == 0
            s.closed_loop_step_dev(B, dx0, do, dg, X, U, u0, cost, status, iters, None, flags=fl, min_margin=margin, ep_flags=flags, ep_steps=steps, stream=q)
            torch.cuda.current_stream().synchronize()
            stepped += alive
            n = g(nsqp)
            assert ((n[alive] >= 1) & (n[alive] <= 3)).all(), n
            assert np.array_equal(g(doff), 2 + stepped), (g(doff), stepped)
        assert bd.intact()
        assert stepped[idle] == 0 and stepped.max() == 3
        for name, d, init in (("x0", dx0, x0), ("obst", do, inp["obst"]), ("X", X, X0), ("U", U, U0), ("u0", u0, np.full((B, 2), -5.0)), ("cost", cost, np.full(B, -5.0)),
                              ("status", status, np.full(B, -9)), ("iters", iters, np.full(B, -9)), ("sqp_iters", nsqp, np.full(B, -77)),
                              ("steps", steps, np.full(B, 100)), ("offset", doff, np.full(B, 2)), ("margin", margin, np.full(B, INF))):
            assert np.array_equal(g(d)[idle], init[idle]), f"the idle instance's {name} was written"
        assert len(set(g(nsqp)[np.arange(B) != idle].tolist())) >= 2, g(nsqp)      # (the step tolerance decided for some instances and not for others)


@pytest.mark.parametrize("cid", FUSED)
def test_fused_step_idle_instance_and_reference_offset(mg, cid):
    on_own_stream(_fused_idle_and_reference, mg, cid)


def _off_means_off(mg):
    mpc_gpu, orc = mg
    N, no = 20, 3
    x0, goal, obst = random_batch(B, no, seed=5)
    with make(mpc_gpu, N, no, B) as fresh:
        name0 = fresh.kernel_name(B)
        want = run(fresh, x0, obst, goal)
    with make(mpc_gpu, N, no, B) as s:
        s.set_sqp(3, 0.0)
        on_name = s.kernel_name(B)
        assert level_of(on_name) == 5 and on_name.endswith(", true" * 5 + ">") and on_name == sc.case("split3-3")["name"]
        on = run(s, x0, obst, goal)
        r = s.solve(x0, obst, goal)
        assert ((r["sqp_iters"] == 3) | (r["status"] == 4)).all() and (r["sqp_iters"] == 3).any(), r      # (step_tol = 0 never stops an instance)
        s.set_sqp(1, 0.0)
        assert s.kernel_name(B) == name0 and level_of(name0) == 0
        assert "sqp_iters" not in s.solve(x0, obst, goal)
        assert_same(run(s, x0, obst, goal), want)
    assert not all(np.array_equal(a[0], b[0]) for a, b in zip(on, want))      # (three iterations are not one)


def test_off_means_off(mg):
    on_own_stream(_off_means_off, mg)


def _names_and_refusals(mg):
    mpc_gpu, orc = mg
    for c in sc.CASES:
        with make(mpc_gpu, c["N"], c["no"], B) as s:
            s.set_sqp(K, 0.0)
            for batch in (1, B):
                assert s.kernel_name(batch) == c["name"] and s.kernel_name(batch, lookahead=False) == c["name"]
    assert len({c["name"] for c in sc.CASES}) == len(sc.CASES)
    # the remaining three of the eleven rows: five obstacles
    for N, name in ((20, "rti_split_kernel<5, 3, false, true, false"), (30, "rti_split_kernel<5, 2, false, true, false"), (50, "rti_solve_kernel<5, 64, 3, true")):
        with make(mpc_gpu, N, 5, B) as s:
            s.set_sqp(2, INF)
            assert s.kernel_name(B) == name + ", true" * 5 + ">"
    x0, goal, obst = random_batch(B, 3, seed=5)
    refusals = (("matrix cores", lambda s: s.set_matrix_cores(True)), ("systolic sweeps", lambda s: s.set_row_parallel(False)),
                ("block-2 recursions", lambda s: s.set_block_riccati(True)), ("16 lanes", lambda s: s.set_lanes_per_instance(16)),
                ("21 lanes", lambda s: s.set_lanes_per_instance(21)), ("32 lanes", lambda s: s.set_lanes_per_instance(32)))
    for what, setter in refusals:
        with make(mpc_gpu, 10, 3, B) as s:      # (N = 10: 16 lanes hold an instance)
            s.reset_guess(x0)
            setter(s)
            s.solve(x0, obst, goal)      # (without the feature the mapping runs)
            s.set_sqp(2, 0.0)
            with pytest.raises(mpc_gpu.MpcError, match="error -1"):
                s.solve(x0, obst, goal)
            s.set_sqp(1, 0.0)
            s.solve(x0, obst, goal)


def test_kernel_names_and_refusals(mg):
    on_own_stream(_names_and_refusals, mg)


def _argument_validation(mg):
    mpc_gpu, orc = mg
    with make(mpc_gpu, 20, 3, B) as s:
        name0 = s.kernel_name(B)
        for max_iter, tol, field in ((0, 0.0, "max_iter"), (-3, 0.0, "max_iter"), (mpc_gpu._lib.MAX_SQP_ITER + 1, 0.0, "max_iter"),
                                     (3, float("nan"), "step_tol"), (3, -1e-9, "step_tol"), (3, -INF, "step_tol")):
            with pytest.raises(mpc_gpu.MpcError, match=field):
                s.set_sqp(max_iter, tol)
            assert s.kernel_name(B) == name0      # nothing was switched on
        for max_iter, tol in ((2, 0.0), (mpc_gpu._lib.MAX_SQP_ITER, INF), (3, 1e-3)):
            s.set_sqp(max_iter, tol)
            assert level_of(s.kernel_name(B)) == 5
        s.set_sqp()
        assert s.kernel_name(B) == name0
        with pytest.raises(ValueError):
            s.set_sqp_iters_out(np.zeros(B, np.int32))


def test_set_sqp_argument_validation(mg):
    on_own_stream(_argument_validation, mg)


def _pipelined(mg):
    """PipelinedMpc.set_sqp / set_sqp_iters_out: two sub-batches on their own streams give what one handle gives, and each writes its slice of the counts"""
    import torch
    from mpc_gpu import _lib
    from mpc_gpu.pipeline import PipelinedMpc
    mpc_gpu, orc = mg
    c = sc.case("split3-3")
    inp, x0 = _fused_inputs(orc, c)
    N, no = inp["N"], inp["no"]
    dev = torch.device("cuda:0")
    tt = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)
    fl = _lib.STEP_SHIFT | _lib.STEP_PLANT | _lib.STEP_OBSTACLES
    out = []
    for piped in (False, True):
        s = PipelinedMpc(N, no, 0.1 * N, max_batch=B, streams=2) if piped else make(mpc_gpu, N, no, B)
        tx, to, tg = tt(x0), tt(inp["obst"]), tt(inp["goal"])
        X = torch.zeros((B, N + 1, 5), dtype=torch.float64, device=dev); U = torch.zeros((B, N, 2), dtype=torch.float64, device=dev)
        u0 = torch.zeros((B, 2), dtype=torch.float64, device=dev)
        status = torch.zeros(B, dtype=torch.int32, device=dev); iters = torch.zeros(B, dtype=torch.int32, device=dev)
        nsqp = torch.full((B,), -77, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        s.set_sqp(3, c["step_tol"])
        s.set_sqp_iters_out(nsqp)
        assert s.kernel_name(B) == c["name"]
        kw = {} if piped else dict(stream=torch.cuda.current_stream().cuda_stream)
        if piped:
            s.fork()
        s.reset_guess_dev(B, tx, X, U, **kw)
        for _ in range(2):
            s.closed_loop_step_dev(B, tx, to, tg, X, U, u0, None, status, iters, flags=fl, **kw)
        if piped:
            s.join()
        torch.cuda.synchronize()
        out.append([a.cpu().numpy() for a in (tx, to, X, U, u0, status, iters, nsqp)])
        if piped:
            s.set_sqp(); s.set_sqp_iters_out(None)
            assert level_of(s.kernel_name(B)) == 0
        s.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    n = out[1][-1]
    assert ((n >= 1) & (n <= 3)).all() and len(set(n.tolist())) >= 2, n


def test_pipelined_handles_pass_the_setting_through(mg):
    on_own_stream(_pipelined, mg)
