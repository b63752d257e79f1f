"""Per-stage reference trajectories (mpc_set_reference, BatchedMpc.set_reference, MPC_STEP_ADVANCE_REF, the shim's stage_yref mode) on the GPU:
a goal-equivalent reference is bit for bit the goal path on every REF instantiation, non-trivial references match the exact QP shifted to them,
the fused closed loop with an advancing window equals host-driven steps, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from feature_loop import assert_same, mg, on_own_stream, run, smooth_path
from helpers import exact_qp, oracle_P, random_batch, step_vector
from reference_qp import goal_rows, ls_cost, shift_gradient, slack_penalty, stage_gradient, stage_rows

pytestmark = pytest.mark.gpu


def goal_ref(goal, T):
    """yref rows equal to what the solver derives from the goal: [g_x, g_y, 0, 0, 0, 0]"""
    R = np.zeros((goal.shape[0], T, 6))
    R[:, :, :2] = goal[:, None, :]
    return R


def assert_close(a, b):
    for (Xa, Ua, _, ca, sa, _), (Xb, Ub, _, cb, sb, _) in zip(a, b):
        both = (sa == 0) & (sb == 0)
        assert both.mean() >= 0.9
        dx = np.abs(Xa[both] - Xb[both]).reshape(both.sum(), -1).max(axis=1)
        du = np.abs(Ua[both] - Ub[both]).reshape(both.sum(), -1).max(axis=1)
        assert (dx <= 1e-6).mean() >= 0.99 and (du <= 8e-6).mean() >= 0.99


# (N, n_obst, B, lanes_per_stage, waves_per_simd, lanes_per_instance, expected kernel name); Bbig: above the split crossover of 1024 SIMDs
EQUIV = [
    (20, 3, 8, 0, 0, 0, "rti_split_kernel<3, 3, false, false, false, true>"),
    (20, 3, 8, 2, 0, 0, "rti_split_kernel<3, 2, false, false, false, true>"),
    (20, 3, 8, 0, 2, 0, "rti_split_kernel<3, 3, true, false, false, true>"),
    (20, 3, 9000, 0, 0, 0, "rti_split_kernel<3, 3, true, false, false, true>"),
    (20, 5, 8, 0, 0, 0, "rti_split_kernel<5, 3, false, false, false, true>"),
    (20, 5, 8, 0, 2, 0, "rti_split_kernel<5, 3, true, false, false, true>"),
    (30, 10, 8, 0, 0, 0, "rti_split_kernel<10, 2, false, false, false, true>"),
    (30, 10, 8, 0, 2, 0, "rti_split_kernel<10, 2, true, false, false, true>"),
    (20, 4, 8, 0, 0, 0, "rti_split_kernel<5, 3, false, true, false, true>"),
    (30, 7, 8, 0, 0, 0, "rti_split_kernel<10, 2, false, true, false, true>"),
    (30, 2, 8, 0, 0, 0, "rti_split_kernel<3, 2, false, true, false, true>"),
    (20, 3, 8, 1, 0, 0, "rti_solve_kernel<3, 64, 3, false, true>"),
    (20, 5, 8, 0, 0, 64, "rti_solve_kernel<5, 64, 3, false, true>"),
    (50, 10, 8, 0, 0, 0, "rti_solve_kernel<10, 64, 3, false, true>"),
    (40, 3, 8, 0, 0, 0, "rti_solve_kernel<3, 64, 3, false, true>"),
    (40, 2, 8, 0, 0, 0, "rti_solve_kernel<3, 64, 3, true, true>"),
    (62, 8, 8, 0, 0, 0, "rti_solve_kernel<10, 64, 3, true, true>"),
    (20, 15, 8, 0, 0, 0, "rti_wide_kernel<20, 2, true, true>"),
    (20, 20, 8, 0, 0, 0, "rti_wide_kernel<20, 2, false, true>"),
    (31, 32, 8, 0, 0, 0, "rti_wide_kernel<32, 2, false, true>"),
    (10, 25, 8, 0, 0, 0, "rti_wide_kernel<32, 2, true, true>"),
]


def make(mpc_gpu, N, no, Tf, B, lps, waves, lpi):
    s = mpc_gpu.BatchedMpc(N, no, Tf, max_batch=B)
    s.set_instance_scheduling(False)      # (the launch order then depends on nothing but the batch: the calls below may differ in history)
    if lps:
        s.set_lanes_per_stage(lps)
    if waves:
        s.set_waves_per_simd(waves)
    if lpi:
        s.set_lanes_per_instance(lpi)
    return s


@pytest.mark.parametrize("N,no,B,lps,waves,lpi,name", EQUIV)
def test_goal_equivalent_reference_is_bit_identical(mg, N, no, B, lps, waves, lpi, name):
    mpc_gpu, orc = mg
    Tf = 0.1 * N
    x0, goal, obst = random_batch(B, no, seed=7 * N + no + B)
    cfg = orc.config(N, no, Tf)
    with make(mpc_gpu, N, no, Tf, B, lps, waves, lpi) as a, make(mpc_gpu, N, no, Tf, B, lps, waves, lpi) as r:
        r.set_reference(goal_ref(goal, N + 1))
        assert r.kernel_name(B) == name
        # the goal path runs the same instantiation without REF: bit for bit; where the reference path keeps a narrower dispatch (the split mapping
        # beyond the crossover, one instance per wavefront on compact blocks) it is compared with the goal path's own kernel within the parity tolerance
        same = a.kernel_name(B)[:-1] + ", true>" == name
        # (the REF cost is formed from residuals against row values the compiler cannot see are the goal's, and its contraction into fused multiply-adds
        # may differ from the goal path's: the reported cost to the last bits)
        check = (lambda p, q: assert_same(p, q, cost_rtol=1e-13)) if same else assert_close
        # look-ahead in the kernel (obstacle states)
        check(run(a, x0, obst, goal), run(r, x0, obst, goal))
        # explicit P (host path)
        P = oracle_P(orc, cfg, obst)
        check(run(a, x0, P, goal, 2), run(r, x0, P, goal, 2))
        # a reference that clamps (T = 1, offset past the end) is the same reference, bit for bit on the same kernel
        ref_runs = run(r, x0, obst, goal, 2)
        r.set_reference(goal_ref(goal, 1), offset=np.full(B, 5, np.int32))
        r.reset_guess(x0)
        assert_same(ref_runs, run(r, x0, obst, goal, 2), cost_rtol=1e-13)
        # cleared: the goal path again, same kernel family as a handle that never had one
        r.set_reference(None)
        assert r.kernel_name(B) == a.kernel_name(B)
        assert_same(run(a, x0, obst, goal, 2), run(r, x0, obst, goal, 2), cost_rtol=1e-13)


def _body_goal_equivalent_reference_fused_step(mg, N, no, B):
    """the fused closed-loop step (device API): bit for bit the same with a goal-equivalent device reference"""
    import torch
    mpc_gpu, _ = mg
    Tf = 0.1 * N
    x0, goal, obst = random_batch(B, no, seed=99 + N + no)
    dev = torch.device("cuda", 0)
    res = []
    for use_ref in (False, True):
        with mpc_gpu.BatchedMpc(N, no, Tf, max_batch=B) as s:
            tx = torch.tensor(x0, device=dev); to = torch.tensor(obst, device=dev); tg = torch.tensor(goal, device=dev)
            X = torch.zeros((B, N + 1, 5), dtype=torch.float64, device=dev); U = torch.zeros((B, N, 2), dtype=torch.float64, device=dev)
            u0 = torch.zeros((B, 2), dtype=torch.float64, device=dev); cost = torch.zeros(B, dtype=torch.float64, device=dev)
            st = torch.zeros(B, dtype=torch.int32, device=dev); it = torch.zeros(B, dtype=torch.int32, device=dev)
            yref = torch.tensor(goal_ref(goal, N + 1), device=dev)
            off = torch.zeros(B, dtype=torch.int32, device=dev)
            if use_ref:
                s.set_reference(yref, off)
            s.reset_guess_dev(B, tx, X, U, stream=torch.cuda.current_stream().cuda_stream)
            for _ in range(6):
                flags = mpc_gpu._lib.STEP_SHIFT | mpc_gpu._lib.STEP_PLANT | mpc_gpu._lib.STEP_OBSTACLES
                s.closed_loop_step_dev(B, tx, to, tg, X, U, u0, cost, st, it, flags=flags, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            res.append([t.cpu().numpy() for t in (tx, to, X, U, u0, cost, st, it)])
    for k, (p, q) in enumerate(zip(*res)):
        assert np.array_equal(p, q) if k != 5 else np.allclose(p, q, rtol=1e-13, atol=0.0)


NONTRIV = [(20, 3, 16), (50, 10, 8), (20, 15, 8), (30, 5, 8)]


def _body_nontrivial_reference_against_exact_qp(mg, N, no, B):
    """random smooth paths, a terminal row of their own, per-instance offsets (some past T: they clamp): the RTI step is the exact solution of
    the QP whose gradient is shifted to the reference; the cost is the LS cost against it plus the exact penalty; the linearisation's q is the
    numpy gradient"""
    import torch
    mpc_gpu, orc = mg
    Tf = 0.1 * N
    rng = np.random.default_rng(1000 + N + no)
    x0, goal, obst = random_batch(B, no, seed=31 + N + no)
    x0[:, 3:] = 0.0
    T = N + 6
    yref = smooth_path(rng, B, T)
    off = rng.integers(0, 4, B).astype(np.int32); off[0] = 0; off[-1] = T + 3
    cfg = orc.config(N, no, Tf)
    P = oracle_P(orc, cfg, obst)
    with mpc_gpu.BatchedMpc(N, no, Tf, max_batch=B) as s:
        s.reset_guess(x0)
        X0, U0 = s.get_traj(B)
        s.set_reference(yref, offset=off)
        out = s.solve(x0, P, goal)
        X, U = s.get_traj(B)
        # linearisation at the returned iterate, against the reference
        dev = torch.device("cuda", 0)
        t = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)
        z = lambda *sh: torch.zeros(sh, dtype=torch.float64, device=dev)
        q = z(B, N + 1, 7)
        s.linearize_dev(B, t(x0), t(P), t(goal), t(X), t(U), z(B, N, 5, 5), z(B, N, 5, 2), z(B, N, 5), q, z(B, N + 1, no), z(B, N + 1, no, 2), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        q = q.cpu().numpy()
    checked = 0
    for b in range(B):
        R = stage_rows(yref[b], off[b], N)
        assert np.abs(q[b] - stage_gradient(cfg, X[b], U[b], R)).max() <= 1e-12
        J = ls_cost(cfg, X[b], U[b], R) + slack_penalty(cfg, x0[b], goal[b], X[b], P[b])
        assert abs(out["cost"][b] - J) <= 1e-10 * max(1.0, abs(J)), (b, out["cost"][b], J)
        if out["status"][b] != 0:
            continue
        qp = shift_gradient(cfg, orc.export_qp(cfg, x0[b], P[b], goal[b], X0[b], U0[b]), goal[b], R)
        v, ok, info = exact_qp(qp, step_vector(N, X0[b], U0[b], X[b], U[b]))
        if not ok:
            continue
        assert np.abs(v - step_vector(N, X0[b], U0[b], X[b], U[b])).max() <= 1e-6, (b, info)
        checked += 1
    assert (out["status"] == 0).mean() >= 0.75, out["status"]
    assert checked >= B // 2


def _body_closed_loop_advancing_window(mg):
    """20 fused steps with ADVANCE_REF | SHIFT | PLANT | OBSTACLES equal 20 host-driven steps (solve, plant step, shift) with the window
    path[i : i + N + 1] set each step; with the episode bookkeeping, instances that reached the goal stop advancing"""
    import torch
    mpc_gpu, _ = mg
    L = mpc_gpu._lib
    N, no, B, steps = 20, 3, 8, 20
    Tf = 2.0
    rng = np.random.default_rng(5)
    x0, goal, obst = random_batch(B, no, seed=55)
    path = smooth_path(rng, B, steps + N + 1)
    dev = torch.device("cuda", 0)
    # fused, device resident
    with mpc_gpu.BatchedMpc(N, no, Tf, max_batch=B) as s:
        tx = torch.tensor(x0, device=dev); to = torch.tensor(obst, device=dev); tg = torch.tensor(goal, device=dev)
        X = torch.zeros((B, N + 1, 5), dtype=torch.float64, device=dev); U = torch.zeros((B, N, 2), dtype=torch.float64, device=dev)
        u0 = torch.zeros((B, 2), dtype=torch.float64, device=dev); st = torch.zeros(B, dtype=torch.int32, device=dev)
        ty = torch.tensor(path, device=dev); toff = torch.zeros(B, dtype=torch.int32, device=dev)
        s.set_reference(ty, toff)
        s.reset_guess_dev(B, tx, X, U, stream=torch.cuda.current_stream().cuda_stream)
        us = []
        for _ in range(steps):
            s.closed_loop_step_dev(B, tx, to, tg, X, U, u0, None, st, None, flags=L.STEP_ADVANCE_REF | L.STEP_SHIFT | L.STEP_PLANT | L.STEP_OBSTACLES, stream=torch.cuda.current_stream().cuda_stream)
            us.append(u0.cpu().numpy().copy())
        torch.cuda.synchronize()
        fused = (tx.cpu().numpy(), X.cpu().numpy(), U.cpu().numpy(), np.array(us))
        assert np.array_equal(toff.cpu().numpy(), np.full(B, steps, np.int32))
    # host-driven: solve_dev + plant step + shift, the window copied each step
    with mpc_gpu.BatchedMpc(N, no, Tf, max_batch=B) as s:
        tx = torch.tensor(x0, device=dev); to = torch.tensor(obst, device=dev); tg = torch.tensor(goal, device=dev)
        X = torch.zeros((B, N + 1, 5), dtype=torch.float64, device=dev); U = torch.zeros((B, N, 2), dtype=torch.float64, device=dev)
        u0 = torch.zeros((B, 2), dtype=torch.float64, device=dev); st = torch.zeros(B, dtype=torch.int32, device=dev)
        win = torch.zeros((B, N + 1, 6), dtype=torch.float64, device=dev)
        s.set_reference(win)
        s.reset_guess_dev(B, tx, X, U, stream=torch.cuda.current_stream().cuda_stream)
        P = torch.zeros((B, N + 1, no, 2), dtype=torch.float64, device=dev)
        xn = torch.zeros_like(tx)
        us = []
        for i in range(steps):
            win.copy_(torch.tensor(path[:, i:i + N + 1], device=dev))
            s.closed_loop_step_dev(B, tx, to, tg, X, U, u0, None, st, None, flags=L.STEP_SHIFT | L.STEP_PLANT | L.STEP_OBSTACLES, stream=torch.cuda.current_stream().cuda_stream)
            us.append(u0.cpu().numpy().copy())
        torch.cuda.synchronize()
        host = (tx.cpu().numpy(), X.cpu().numpy(), U.cpu().numpy(), np.array(us))
    for p, q in zip(fused, host):
        assert np.array_equal(p, q)
    # bookkeeping: an instance that starts at its goal idles, its offset stays
    with mpc_gpu.BatchedMpc(N, no, Tf, max_batch=B) as s:
        x1 = x0.copy(); x1[0, :2] = goal[0]; x1[0, 3:] = 0.0
        tx = torch.tensor(x1, device=dev); to = torch.tensor(obst, device=dev); tg = torch.tensor(goal, device=dev)
        X = torch.zeros((B, N + 1, 5), dtype=torch.float64, device=dev); U = torch.zeros((B, N, 2), dtype=torch.float64, device=dev)
        mm = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
        fl = torch.zeros(B, dtype=torch.int32, device=dev); ns = torch.zeros(B, dtype=torch.int32, device=dev)
        ty = torch.tensor(path, device=dev); toff = torch.zeros(B, dtype=torch.int32, device=dev)
        s.set_reference(ty, toff)
        s.reset_guess_dev(B, tx, X, U, stream=torch.cuda.current_stream().cuda_stream)
        flags = L.STEP_ADVANCE_REF | L.STEP_SHIFT | L.STEP_PLANT | L.STEP_OBSTACLES | L.STEP_METRICS
        for _ in range(3):
            s.closed_loop_step_dev(B, tx, to, tg, X, U, flags=flags, min_margin=mm, ep_flags=fl, ep_steps=ns, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        off, f = toff.cpu().numpy(), fl.cpu().numpy()
        assert f[0] & 1 and off[0] == 1          # reached in its first step: that step advanced, the idle ones did not
        assert all(off[b] == 3 for b in range(B) if not f[b] & 1)


def test_refusals(mg):
    mpc_gpu, _ = mg
    L = mpc_gpu._lib
    N, no, B = 20, 3, 4
    x0, goal, obst = random_batch(B, no, seed=3)
    for setup in (lambda s: s.set_matrix_cores(True), lambda s: s.set_row_parallel(False), lambda s: s.set_block_riccati(True),
                  lambda s: s.set_lanes_per_instance(32)):
        with mpc_gpu.BatchedMpc(N, no, 2.0, max_batch=B) as s:
            setup(s)
            s.set_reference(goal_ref(goal, N + 1))
            with pytest.raises(mpc_gpu.MpcError, match="per-stage reference"):
                s.solve(x0, obst, goal)
    with mpc_gpu.BatchedMpc(N, no, 2.0, max_batch=B) as s:
        h = s._h
        ok = goal_ref(goal, N + 1)
        assert L.lib().mpc_set_reference(h, B, 0, ok.ctypes.data, None) == L.MPC_ERR_ARG
        assert L.lib().mpc_set_reference(h, B + 1, N + 1, np.zeros((B + 1, N + 1, 6)).ctypes.data, None) == L.MPC_ERR_ARG
        bad = ok.copy(); bad[1, 3, 2] = np.nan
        assert L.lib().mpc_set_reference(h, B, N + 1, bad.ctypes.data, None) == L.MPC_ERR_ARG
        neg = np.array([0, -1, 0, 0], np.int32)
        assert L.lib().mpc_set_reference(h, B, N + 1, ok.ctypes.data, neg.ctypes.data) == L.MPC_ERR_ARG
        # ADVANCE_REF without offsets, and without a reference at all
        import torch
        dev = torch.device("cuda", 0)
        tx = torch.tensor(x0, device=dev); to = torch.tensor(obst, device=dev); tg = torch.tensor(goal, device=dev)
        X = torch.zeros((B, N + 1, 5), dtype=torch.float64, device=dev); U = torch.zeros((B, N, 2), dtype=torch.float64, device=dev)
        for with_ref in (False, True):
            if with_ref:
                s.set_reference(ok)
            with pytest.raises(mpc_gpu.MpcError, match="ADVANCE_REF"):
                s.closed_loop_step_dev(B, tx, to, tg, X, U, flags=L.STEP_ADVANCE_REF | L.STEP_PLANT)
        # a reference for fewer instances than the solve
        s.set_reference(ok[:2])
        with pytest.raises(mpc_gpu.MpcError, match="fewer instances"):
            s.solve(x0, obst, goal)


def test_shim_stage_yref_matches_set_reference(mg):
    """acados-style per-stage cost_set(i, 'yref') through the shim is bit for bit BatchedMpc.set_reference on the same rows"""
    mpc_gpu, orc = mg
    N, no = 20, 5
    rng = np.random.default_rng(8)
    x0, goal, obst = random_batch(1, no, seed=8)
    cfg = orc.config(N, no, 2.0)
    P = oracle_P(orc, cfg, obst)
    R = smooth_path(rng, 1, N + 1)[0]
    R[N, 4:] = 0.0
    shim = mpc_gpu.AcadosOcpSolverShim(N, no, 2.0, goal=goal[0], x0=x0[0], stage_yref=True)
    for i in range(N):
        shim.cost_set(i, "yref", R[i])
    shim.cost_set(N, "yref", R[N, :4])
    for i in range(N + 1):
        shim.set(i, "p", P[0, i].reshape(-1))
    shim.set(0, "lbx", x0[0]); shim.set(0, "ubx", x0[0])
    for i in range(N + 1):
        shim.set(i, "x", np.array([x0[0, 0], x0[0, 1], x0[0, 2], 0.0, 0.0]))
    st = shim.solve()
    with mpc_gpu.BatchedMpc(N, no, 2.0, max_batch=1) as s:
        s.reset_guess(x0)
        s.set_reference(R[None])
        o = s.solve(x0, P, goal)
        X, U = s.get_traj(1)
    assert st == o["status"][0] and shim.cost == o["cost"][0]      # (the same REF kernel on both sides: the cost too is bit for bit)
    assert np.array_equal(shim.X, X[0]) and np.array_equal(shim.U, U[0])
    shim.mpc.close()


@pytest.mark.parametrize("N,no,B", [(20, 3, 8), (30, 10, 4), (20, 15, 4), (50, 10, 4)])
def test_goal_equivalent_reference_fused_step(mg, N, no, B):
    """the fused closed-loop step (device API): bit for bit the same with a goal-equivalent device reference"""
    on_own_stream(_body_goal_equivalent_reference_fused_step, mg, N, no, B)


@pytest.mark.parametrize("N,no,B", NONTRIV)
def test_nontrivial_reference_against_exact_qp(mg, N, no, B):
    """random smooth paths against the exact QP shifted to them, cost and linearisation (see the body)"""
    on_own_stream(_body_nontrivial_reference_against_exact_qp, mg, N, no, B)


def test_closed_loop_advancing_window(mg):
    """20 fused steps with ADVANCE_REF equal 20 steps with the window set each step; idle instances do not advance (see the body)"""
    on_own_stream(_body_closed_loop_advancing_window, mg)
