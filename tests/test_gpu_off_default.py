"""Every kernel family at a time step dt = Tf / N that is not 0.1 and at world constants that are not the reference's (off_default_cases.py: the rows,
OFF, scaled_batch, wall_cases; test_off_default_host.py pins the oracle there and asserts the oracle-alone counts the rows store).
  1. linearisation, plant step, look-ahead and ground-truth obstacle motion against the oracle's functions;
  2. the look-ahead inside every row's solve kernel == the look-ahead given as P, bit for bit, on obstacles that meet all four walls of OFF's arena;
  3. three solves of every row x {default constants, OFF} under helpers.judge_against_oracle, the kernel named in the table asserted first;
  4. the six acados switches on four rows at the rows' own steps;
  5. the fused control step against helpers.OracleLoop on the four solve tails, with a robot that reaches its goal and one that leaves OFF's arena;
  6. the feature levels (instance parameters in host and device form, obstacle mask, instance bounds) at two rows.
Every tolerance is one the suite already asserts; each test prints the figures it judged."""
import numpy as np
import pytest

import off_default_cases as oc
from feature_loop import GpuLoop, assert_same, mg, on_own_stream
from helpers import OracleLoop, adjudicate, judge_against_oracle, oracle_P

pytestmark = pytest.mark.gpu

ROW_IDS = [r["id"] for r in oc.ROWS]


def gpu_three_solves(s, ref, x0, obst, P, goal):
    """the three solves of oracle_three_solves on the handle: a cold start (reset_guess), then two from the oracle's shifted iterate (set_warmstart);
    the first and third take obstacle states (look-ahead in the kernel), the second the explicit P.  Returns [(g, X, U)]."""
    B = x0.shape[0]
    outs = []
    for k, (X0, U0, _) in enumerate(ref):
        if k == 0:
            s.reset_guess(x0)
        else:
            s.set_warmstart(X0, U0)
        g = s.solve(x0, P if k == 1 else obst, goal)
        X, U = s.get_traj(B)
        outs.append((g, X, U))
    return outs


def judge_solves(orc, cfg, ref, outs, x0, P, goal, counts, capped, what):
    """section 3's judgement of every solve: helpers.judge_against_oracle with its own tolerances, no status borderline unless the oracle's run reached
    the cap, the table's count of converged instances, the median |X_gpu - X_oracle| of test_wide_solve_parity"""
    for k, ((X0, U0, o), (g, X, U)) in enumerate(zip(ref, outs)):
        n = judge_against_oracle(orc, cfg, x0, P, goal, X0, U0, g, X, U, o)
        ok = (o["status"] == 0) & (g["status"] == 0)
        med = float(np.median(np.abs(X - o["X"]).reshape(len(x0), -1).max(1)[ok])) if ok.any() else 0.0
        print(f"OFFDEFAULT {what} solve {k + 1}: converged {n['converged']} worst_gpu_oracle {n['worst_d_gpu_oracle']:.3e} median {med:.3e} "
              f"adjudicated {n['judged_by_qp']} worst_gpu_exact {n['worst_d_gpu_exact']:.3e} worst_oracle_exact {n['worst_d_oracle_exact']:.3e} "
              f"status_borderline {n['status_borderline']} iter_borderline {n['iter_borderline']}")
        if not capped:
            assert n["status_borderline"] == 0, (what, k, n)
        assert n["converged"] == counts[k], (what, k, n, counts)
        assert med < 1e-9, (what, k, med)


def as_runs(outs):
    """[(g, X, U)] in the record layout of feature_loop.run, for assert_same"""
    return [(X, U, g["u0"], g["cost"], g["status"], g["iters"]) for g, X, U in outs]


# ---------------------------------------------------------------------------------------------------------------- 1. linearisation, plant, look-ahead
def _body_linearize(mg, N, no, dt):
    import torch
    mpc_gpu, orc = mg
    B, Tf = 8, dt * N
    x0, goal, obst = oc.scaled_batch(B, no, 3, oc.OFF["arena"])
    cfg = orc.config(N, no, Tf, **oc.OFF)
    h = cfg.Tf / cfg.N
    P = oracle_P(orc, cfg, obst)
    rng = np.random.default_rng(5)
    X = rng.uniform(-7, 7, (B, N + 1, 5)); X[:, :, 2] = rng.uniform(-6, 6, (B, N + 1)); U = rng.uniform(-8, 8, (B, N, 2))
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
    with mpc_gpu.BatchedMpc(N, no, Tf, max_batch=B, **oc.OFF) as s:
        A, Bm, b, q, hv, dh = z(B, N, 5, 5), z(B, N, 5, 2), z(B, N, 5), z(B, N + 1, 7), z(B, N + 1, no), z(B, N + 1, no, 2)
        torch.cuda.synchronize()
        s.linearize_dev(B, t(x0), t(P), t(goal), t(X), t(U), A, Bm, b, q, hv, dh, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        x = np.column_stack([rng.uniform(-7, 7, (B, 2)), rng.uniform(-6, 6, B), rng.uniform(-10, 10, (B, 2))]); u = rng.uniform(-8, 8, (B, 2))
        xn = s.plant_step(x, u)
    for i in range(B):
        ref = orc.linearize(cfg, x0[i], P[i], goal[i], X[i], U[i])
        for name, got in (("A", A), ("B", Bm), ("b", b), ("q", q), ("h", hv), ("dh", dh)):
            assert np.abs(got[i].cpu().numpy() - ref[name]).max() <= 1e-12 * max(1.0, np.abs(ref[name]).max()), (name, i)
    # the entries that are the step itself (the oracle's are pinned against finite differences by the host test)
    Ag, Bg = A.cpu().numpy(), Bm.cpu().numpy()
    assert np.allclose(Ag[:, :, 2, 4], h, rtol=1e-15) and np.allclose(Bg[:, :, 3, 0], h, rtol=1e-15) and np.allclose(Bg[:, :, 2, 1], 0.5 * h * h, rtol=1e-14)
    want = np.stack([orc.dynamics(x[i], u[i], h)[0] for i in range(B)])
    assert np.abs(xn - want).max() < 1e-13


@pytest.mark.parametrize("dt", [0.05, 0.16])
@pytest.mark.parametrize("N,no", [(20, 3), (5, 1)])
def test_linearisation_and_plant_step(mg, N, no, dt):
    on_own_stream(_body_linearize, mg, N, no, dt)


def _body_lookahead(mg, N, dt):
    import torch
    mpc_gpu, orc = mg
    no, B, steps = 3, 6, 8
    arena = oc.OFF["arena"]
    _, _, obst, hits = oc.wall_cases(B, no, 60 + N, arena, dt)
    for bug in (1, 0):
        cfg = orc.config(N, no, dt * N, arena=arena, bug_compat_predict=bug)
        want = np.stack([orc.predict_params(cfg, o) for o in obst])
        with mpc_gpu.BatchedMpc(N, no, dt * N, max_batch=B, arena=arena, bug_compat_predict=bug) as s:
            P = s.predict(obst)
        assert np.array_equal(P, want), bug
        d = np.diff(P, axis=1)
        assert ((d.max(axis=1) > 0) & (d.min(axis=1) < 0)).any(), "no reflection inside the horizon"
        assert (P[:, 0, :, 0] == arena[1]).any()                        # one obstacle starts exactly on xmax
    # the ground-truth motion (x moves with vx), `steps` steps running, without and with velocity noise
    cfg = orc.config(N, no, dt * N, arena=arena)
    step = cfg.Tf / cfg.N
    dev = torch.device("cuda:0")
    noise = np.random.default_rng(int(1000 * dt) + N).standard_normal((steps, B * no, 2))
    with mpc_gpu.BatchedMpc(N, no, dt * N, max_batch=B, arena=arena) as s:
        for noisy in (False, True):
            st = torch.from_numpy(obst.reshape(B * no, 4).copy()).to(dev)
            ref = obst.reshape(B * no, 4).copy()
            turned = False
            for k in range(steps):
                nz = torch.from_numpy(noise[k].copy()).to(dev) if noisy else None
                torch.cuda.synchronize()
                s.obstacle_step_dev(B * no, st, nz, 0.1, 2.0, stream=torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                new = np.stack([orc.obstacle_step(cfg, ref[i], step, noise[k, i] if noisy else None, 0.1, 2.0) for i in range(B * no)])
                turned = turned or bool((np.sign(new[:, 2:]) != np.sign(ref[:, 2:])).any())
                ref = new
                assert np.array_equal(st.cpu().numpy(), ref), (noisy, k)
            assert turned


@pytest.mark.parametrize("dt", [0.05, 0.07, 0.16, 0.25])
@pytest.mark.parametrize("N", [5, 20, 21, 50])
def test_lookahead_and_obstacle_motion_are_the_oracles(mg, N, dt):
    """predict (with the defect D1 and without) and obstacle_step_dev (without and with noise) under OFF's arena on the wall cases, bit for bit"""
    on_own_stream(_body_lookahead, mg, N, dt)


# ---------------------------------------------------------------------------------------------------------------- 2. look-ahead in the solve kernel
@pytest.mark.parametrize("rid", ROW_IDS)
def test_lookahead_in_the_kernel_is_the_lookahead_given(mg, rid):
    mpc_gpu, _ = mg
    row = oc.ROW[rid]
    N, no, B, Tf = row["N"], row["no"], row["B"], row["Tf"]
    x0, goal, obst, _ = oc.wall_cases(B, no, row["seed"], oc.OFF["arena"], Tf / N)
    res = {}
    for how in ("obst", "P"):
        with mpc_gpu.BatchedMpc(N, no, Tf, max_batch=B, **oc.OFF) as s:
            oc.configure(s, row)
            P = s.predict(obst)
            if how == "P" and N >= 3:
                d = np.diff(P, axis=1)
                assert ((d.max(axis=1) > 0) & (d.min(axis=1) < 0)).any(), "no reflection inside the horizon"
            s.reset_guess(x0)
            g = s.solve(x0, obst if how == "obst" else P, goal)
            X, U = s.get_traj(B)
            res[how] = [(g, X, U)]
    assert_same(as_runs(res["obst"]), as_runs(res["P"]))
    assert (res["obst"][0][0]["status"] == 0).any()


# ---------------------------------------------------------------------------------------------------------------- 3. solve parity
@pytest.mark.parametrize("off", [False, True], ids=["default", "OFF"])
@pytest.mark.parametrize("rid", ROW_IDS)
def test_three_solves_against_the_oracle(mg, rid, off):
    mpc_gpu, orc = mg
    row = oc.ROW[rid]
    N, no, B, Tf = row["N"], row["no"], row["B"], row["Tf"]
    kw = oc.row_cfg(off)
    x0, goal, obst = oc.scaled_batch(B, no, row["seed"], kw.get("arena", oc.DEFAULT_ARENA))
    cfg = orc.config(N, no, Tf, **kw)
    P = oracle_P(orc, cfg, obst)
    ref = oc.oracle_three_solves(orc, cfg, x0, P, goal)
    with mpc_gpu.BatchedMpc(N, no, Tf, max_batch=B, **kw) as s:
        name = oc.configure(s, row)                                     # the kernel name first
        outs = gpu_three_solves(s, ref, x0, obst, P, goal)
    what = f"{rid} {'OFF' if off else 'default'} {name}"
    judge_solves(orc, cfg, ref, outs, x0, P, goal, row["ok_off" if off else "ok_default"], off and row["capped"], what)


# ---------------------------------------------------------------------------------------------------------------- 4. the switches
@pytest.mark.parametrize("rid,sw", oc.switch_cases(), ids=[f"{r}-{sw}" for r, sw in oc.switch_cases()])
def test_switches_away_from_the_default_step(mg, rid, sw):
    """one cold solve with one acados switch off its default, at the row's own Tf (off_default_cases.SWITCH_DROPPED: the pairs left out and why)"""
    mpc_gpu, orc = mg
    row = oc.ROW[rid]
    N, no, B, Tf = row["N"], row["no"], row["B"], row["Tf"]
    kw = {sw: oc.SWITCH_VALUE[sw]}
    x0, goal, obst = oc.scaled_batch(B, no, row["seed"], oc.DEFAULT_ARENA)
    cfg = orc.config(N, no, Tf, **kw)
    P = oracle_P(orc, cfg, obst)
    ref = oc.oracle_three_solves(orc, cfg, x0, P, goal)[:1]
    with mpc_gpu.BatchedMpc(N, no, Tf, max_batch=B, **kw) as s:
        name = oc.configure(s, row)
        outs = gpu_three_solves(s, ref, x0, obst, P, goal)
    judge_solves(orc, cfg, ref, outs, x0, P, goal, [oc.SWITCH_OK[rid][sw]], False, f"{rid} {sw}={kw[sw]} {name}")


# ---------------------------------------------------------------------------------------------------------------- 5. the fused step against the oracle loop
# one row per solve tail (test_gpu_solve_tail.TAILS: one lane per stage, the split kernel's reordered epilogue, its older order, the multi-wavefront kernel)
TAIL_ROWS = {"one-lane": ("g21", "rti_solve_kernel<3, 21"), "split-fx": ("split3", "rti_split_kernel<3, 3, false"),
             "split-w2": ("split3-w2", "rti_split_kernel<5, 3, true"), "wide": ("wide20", "rti_wide_kernel<20")}


@pytest.mark.parametrize("tail", list(TAIL_ROWS))
def test_fused_step_against_the_oracle_loop(mg, tail):
    """test_fused_step_against_the_oracle_loop_with_resync with OFF at the row's step: 8 instances x 6 control steps with velocity noise, the oracle loop
    re-seeded with the GPU's state before every step.  Instance 0 starts 0.05 from its goal (it arrives in the first step and idles); instance 1
    starts 0.1 inside xmax = 9 at v = 3 outwards and leaves OFF's arena, beyond the default arena's wall as well as beyond this one."""
    mpc_gpu, orc = mg
    rid, prefix = TAIL_ROWS[tail]
    row = oc.ROW[rid]
    N, no, Tf, B, K = row["N"], row["no"], row["Tf"], 8, 6
    arena = oc.OFF["arena"]
    x0, goal, obst, _ = oc.wall_cases(B, no, row["seed"], arena, Tf / N)
    goal[0] = x0[0, :2] + [0.05, 0.0]
    x0[1] = [arena[1] - 0.1, 0.5 * (arena[2] + arena[3]) - 3.0, 0.0, 3.0, 0.0]
    noise = np.random.default_rng(88).standard_normal((K, B, no, 2))
    cfg = orc.config(N, no, Tf, **oc.OFF)
    g = GpuLoop(mpc_gpu, N, no, Tf, x0, goal, obst, alias=False, **oc.OFF)
    name = oc.configure(g.m, row, B)
    assert name.startswith(prefix), name
    loops = [OracleLoop(orc, cfg, x0[b], goal[b], obst[b], alias=False) for b in range(B)]
    worst = dict(X=0.0, x=0.0, u=0.0, margin=0.0)
    n_cmp = n_out = 0
    for k in range(K):
        before = g.host()
        for b, L in enumerate(loops):                               # resync: the oracle continues from the GPU's state
            L.x, L.obst = before["x0"][b].copy(), before["obst"][b].copy()
            L.X, L.U = before["X"][b].copy(), before["U"][b].copy()
            L.min_margin, L.flags, L.steps = float(before["margin"][b]), int(before["flags"][b]), int(before["steps"][b])
        g.step(noise[k])
        after = g.host()
        for b, L in enumerate(loops):
            r = L.step(noise[k, b])
            if r is None:                                           # finished episodes idle on both sides
                for key in ("x0", "obst", "X", "U"):
                    assert np.array_equal(after[key][b], before[key][b]), (k, b, key)
                assert after["steps"][b] == before["steps"][b] and after["flags"][b] == before["flags"][b]
                continue
            n_cmp += 1
            assert after["status"][b] == r["status"], (k, b, after["status"][b], r["status"])
            assert np.array_equal(after["obst"][b], L.obst), (k, b)                 # same noise, IEEE-exact obstacle motion
            assert after["flags"][b] == L.flags and after["steps"][b] == L.steps, (k, b, after["flags"][b], L.flags)
            if r["status"] != 0:
                continue                                            # capped / failed QPs: iterates need not agree (the statuses did)
            d = max(np.abs(after["X"][b] - L.X).max(), np.abs(after["U"][b] - L.U).max())
            if d > 1e-6:                                            # adjudicated against the exact solution of the QP, as in the test this one follows
                n_out += 1
                Xn = np.vstack([before["x0"][b][None], after["X"][b][:N]]); Un = np.vstack([after["u0"][b][None], after["U"][b][:N - 1]])
                P = orc.predict_params(cfg, before["obst"][b])
                a = adjudicate(orc, cfg, before["x0"][b], P, goal[b], before["X"][b], before["U"][b], Xn, Un, r["X"], r["U"])
                assert a["passed"], (k, b, d, a)
                continue
            worst["X"] = max(worst["X"], d)
            worst["x"] = max(worst["x"], np.abs(after["x0"][b] - L.x).max())
            worst["u"] = max(worst["u"], np.abs(after["u0"][b] - r["u0"]).max())
            worst["margin"] = max(worst["margin"], abs(after["margin"][b] - L.min_margin))
            assert abs(after["iters"][b] - r["iters"]) <= 1, (k, b)
        if k == 0:
            assert after["flags"][0] & 1 and after["steps"][0] == 0             # arrived in the first step
            assert after["flags"][1] & 2 and after["x0"][1, 0] > arena[1]        # left through xmax
    g.close()
    print(f"OFFDEFAULT fused {tail} {name}: compared {n_cmp} adjudicated {n_out} worst {worst}")
    assert n_cmp > 0.7 * B * K and n_out <= max(2, 0.002 * n_cmp), (n_cmp, n_out)
    assert worst["X"] <= 1e-6 and worst["u"] <= 8e-6 and worst["x"] <= 1e-6 and worst["margin"] <= 1e-6, worst


# ---------------------------------------------------------------------------------------------------------------- 6. the feature levels
def _body_features(mg, rid, form):
    import torch
    mpc_gpu, orc = mg
    row = oc.ROW[rid]
    N, no, B, Tf = row["N"], row["no"], row["B"], row["Tf"]
    world = {k: v for k, v in oc.OFF.items() if k != "r_safe"}          # the handle keeps the default weights and radius: the instance parameters carry IP's
    x0, goal, obst = oc.scaled_batch(B, no, row["seed"], oc.OFF["arena"])
    cfg = orc.config(N, no, Tf, **dict(oc.OFF, **oc.IP))
    P = oracle_P(orc, cfg, obst)
    ref = oc.oracle_three_solves(orc, cfg, x0, P, goal)
    W, We, R = np.tile(oc.IP["W"], (B, 1)), np.tile(oc.IP["We"], (B, 1)), np.full((B, no), oc.IP["r_safe"])
    with mpc_gpu.BatchedMpc(N, no, Tf, max_batch=B, **world) as s:
        s.set_instance_scheduling(False)
        if form == "host":
            s.set_instance_params(W=W, We=We, r_safe=R)
        else:                                                           # device arrays: the tables are derived by instance_params_kernel in front of every solve
            dev = torch.device("cuda:0")
            dW, dWe, dR = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (W, We, R))
            torch.cuda.synchronize()
            s.set_instance_params(W=dW, We=dWe, r_safe=dR)
        name = oc.configure(s, row)
        assert name.endswith(", true, true>"), name
        base = gpu_three_solves(s, ref, x0, obst, P, goal)
        judge_solves(orc, cfg, ref, base, x0, P, goal, oc.FEATURE_OK[rid], False, f"{rid} instance parameters ({form}) {name}")
        # a full obstacle mask on top: the contract of test_full_mask_is_the_instance_parameter_path (the reported cost to 1e-13)
        s.set_obstacle_mask(np.ones((B, no), bool))
        masked = gpu_three_solves(s, ref, x0, obst, P, goal)
        assert s.kernel_name(B).endswith(", true, true, true>"), s.kernel_name(B)
        assert_same(as_runs(base), as_runs(masked), cost_rtol=1e-13)
        # uniform bounds equal to the handle's on top: the contract of test_uniform_bounds_are_the_configured_handle (bit for bit)
        s.set_instance_bounds(bx_lo=list(s.cfg.bx_lo), bx_hi=list(s.cfg.bx_hi), bu_lo=list(s.cfg.bu_lo), bu_hi=list(s.cfg.bu_hi))
        assert s.kernel_name(B).endswith(", true, true, true, true>"), s.kernel_name(B)
        assert_same(as_runs(masked), as_runs(gpu_three_solves(s, ref, x0, obst, P, goal)))


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("rid", sorted(oc.FEATURE_OK))
def test_feature_levels(mg, rid, form):
    on_own_stream(_body_features, mg, rid, form)
