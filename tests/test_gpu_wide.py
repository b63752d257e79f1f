"""11 to 32 obstacles: the multi-wavefront solve kernel (rti_wide_kernel, one instance per workgroup of 2 or 4 wavefronts) against the CPU oracle,
under the contracts the other GPU files use (parity, determinism, the fused closed loop, guard bands), plus the scenario generator for that many
obstacles and the reference's experiment grid (mpc_gpu.run_grid)."""
import glob
import json
import os

import numpy as np
import pytest

from helpers import OracleLoop, adjudicate, adjudicate_batch, oracle_P, oracle_guess, random_batch

pytestmark = pytest.mark.gpu


@pytest.fixture
def mg(built):
    import mpc_gpu
    from oracle import oracle as orc
    mpc_gpu.BatchedMpc.default_lanes_per_stage = 0
    return mpc_gpu, orc


def cap_of(no):
    return 20 if no <= 20 else 32


CASES = [(N, no, B) for N in (2, 10, 20, 30, 31) for no in (11, 15, 20, 21, 30, 32) for B in (7,)] + \
        [(N, no, B) for N, no in ((2, 11), (10, 20), (20, 32), (31, 15), (30, 30)) for B in (1, 64)]


@pytest.mark.parametrize("N,no,B", CASES)
def test_wide_solve_parity(mg, N, no, B):
    """first solve plus two warm-started ones, look-ahead in the kernel and explicit P, against orc.rti_solve_batch (test_any_obstacle_count's judgement)"""
    mpc_gpu, orc = mg
    x0, goal, obst = random_batch(B, no, seed=1000 + 37 * N + no + B)
    Tf = 0.1 * N if N >= 10 else 0.5
    cfg = orc.config(N, no, Tf)
    P = oracle_P(orc, cfg, obst); Xo, Uo = oracle_guess(orc, cfg, x0)
    with mpc_gpu.BatchedMpc(N, no, Tf, max_batch=B) as s:
        name = s.kernel_name(B)
        assert name == f"rti_wide_kernel<{cap_of(no)}, 2, {'false' if no in (20, 32) else 'true'}>", name
        s.reset_guess(x0)
        for k in range(3):
            g = s.solve(x0, obst if k != 1 else P, goal); X, U = s.get_traj(B)
            o = orc.rti_solve_batch(cfg, x0, P, goal, Xo, Uo)
            assert (g["status"] == o["status"]).all(), (k, g["status"], o["status"])
            ok = o["status"] == 0
            if ok.any():
                # iteration counts equal on at least 90 % of the converged instances (one instance of a batch of 7 is 14 %: at most one then)
                assert (g["iters"][ok] != o["iters"][ok]).sum() <= max(1, int(0.1 * ok.sum()))
                d = np.abs(X - o["X"]).reshape(B, -1).max(1)
                adjudicate_batch(orc, cfg, x0, P, goal, Xo, Uo, X, U, o, np.nonzero(ok & (d > 1e-6))[0], what=f"{no} obstacles, N = {N}, step {k}")
                assert np.median(d[ok]) < 1e-9
                rel = np.abs(g["cost"][ok] - o["cost"][ok]) / np.maximum(1.0, np.abs(o["cost"][ok]))
                assert np.median(rel) < 1e-10
            Xo, Uo = o["X"].copy(), o["U"].copy()
            for b in range(B):
                Xo[b], Uo[b] = orc.shift(cfg, Xo[b], Uo[b])
            s.set_warmstart(Xo, Uo)


@pytest.mark.parametrize("N,no", [(20, 15), (31, 32), (10, 25)])
def test_wide_determinism(mg, N, no):
    """the same batch twice: bit-identical; instance b alone: bit-identical to instance b inside a batch of 64 (fixed wave order of every sum)"""
    mpc_gpu, _ = mg
    B = 64
    x0, goal, obst = random_batch(B, no, seed=4 + N + no)
    runs = []
    with mpc_gpu.BatchedMpc(N, no, 0.1 * N, max_batch=B) as s:
        for _ in range(2):
            s.reset_guess(x0)
            g = s.solve(x0, obst, goal); X, U = s.get_traj(B)
            runs.append((g, X, U))
    (ga, Xa, Ua), (gb, Xb, Ub) = runs
    assert np.array_equal(Xa, Xb) and np.array_equal(Ua, Ub)
    for key in ("cost", "status", "iters", "u0"):
        assert np.array_equal(ga[key], gb[key]), key
    for b in (0, 17, 63):
        with mpc_gpu.BatchedMpc(N, no, 0.1 * N, max_batch=1) as s:
            s.reset_guess(x0[b:b + 1])
            g = s.solve(x0[b:b + 1], obst[b:b + 1], goal[b:b + 1]); X, U = s.get_traj(1)
        assert np.array_equal(X[0], Xa[b]) and np.array_equal(U[0], Ua[b]), b
        assert g["cost"][0] == ga["cost"][b] and g["status"][0] == ga["status"][b] and g["iters"][0] == ga["iters"][b], b


@pytest.mark.parametrize("no", [15, 30])
def test_wide_fused_step_against_the_oracle_loop_with_resync(mg, no):
    """test_fused_step_against_the_oracle_loop_with_resync at 15 and 30 obstacles: the reference's RANDOM draws and noise streams, the oracle loop
    re-seeded with the GPU's state before every step; statuses, obstacle states (bit for bit), flags, step counts, margins, iterates"""
    mpc_gpu, orc = mg
    from mpc_gpu.world import reference_streams
    from feature_loop import GpuLoop
    N, Tf, B, K = 20, 2.0, 12, 40
    obst, noise = reference_streams("RANDOM", range(B), no, K)
    x0 = np.tile([-7.0, -7.0, np.pi / 4, 0, 0], (B, 1)); goal = np.tile([7.0, 7.0], (B, 1))
    cfg = orc.config(N, no, Tf)
    g = GpuLoop(mpc_gpu, N, no, Tf, x0, goal, obst)
    assert g.m.kernel_name(B).startswith(f"rti_wide_kernel<{cap_of(no)},")
    loops = [OracleLoop(orc, cfg, x0[b], goal[b], obst[b]) for b in range(B)]
    worst = dict(X=0.0, x=0.0, margin=0.0)
    n_cmp = n_out = 0
    for k in range(K):
        before = g.host()
        for b, L in enumerate(loops):
            L.x, L.obst = before["x0"][b].copy(), before["obst"][b].copy()
            L.X, L.U = before["X"][b].copy(), before["U"][b].copy()
            L.min_margin, L.flags, L.steps = float(before["margin"][b]), int(before["flags"][b]), int(before["steps"][b])
        g.step(noise[k])
        after = g.host()
        for b, L in enumerate(loops):
            r = L.step(noise[k, b])
            if r is None:
                for key in ("x0", "obst", "X", "U"):
                    assert np.array_equal(after[key][b], before[key][b]), (k, b, key)
                continue
            n_cmp += 1
            assert after["status"][b] == r["status"], (k, b, after["status"][b], r["status"])
            assert np.array_equal(after["obst"][b], L.obst), (k, b)
            assert after["flags"][b] == L.flags and after["steps"][b] == L.steps, (k, b)
            if r["status"] != 0:
                continue
            d = max(np.abs(after["X"][b] - L.X).max(), np.abs(after["U"][b] - L.U).max())
            if d > 1e-6:
                n_out += 1
                Xn = np.vstack([before["x0"][b][None], after["X"][b][:N]]); Un = np.vstack([after["u0"][b][None], after["U"][b][:N - 1]])
                P = orc.predict_params(cfg, before["obst"][b])
                a = adjudicate(orc, cfg, before["x0"][b], P, goal[b], before["X"][b], before["U"][b], Xn, Un, r["X"], r["U"])
                # with up to 2 n_obst N active rows the QP can sit at the float64 floor of BOTH interior points: the GPU's step passes below EXACT_CAP, or
                # when it is at least as close to the exact solution as the oracle's
                assert a["passed"] or (a["kind"] == "exact" and a["d_gpu"] <= a["d_oracle"]), (k, b, d, a)
                continue
            worst["X"] = max(worst["X"], d)
            worst["x"] = max(worst["x"], np.abs(after["x0"][b] - L.x).max())
            worst["margin"] = max(worst["margin"], abs(after["margin"][b] - L.min_margin))
    g.close()
    assert n_cmp > 0.5 * B * K and n_out <= max(2, 0.002 * n_cmp), (n_cmp, n_out)
    assert worst["X"] <= 1e-6 and worst["x"] <= 1e-6 and worst["margin"] <= 1e-6, worst


@pytest.mark.parametrize("N,no", [(20, 20), (20, 13), (31, 32), (31, 27)])
def test_wide_guard_bands(mg, N, no):
    """every new instantiation takes one fused step with every optional output wired to guard-banded arrays: bands intact, accumulators equal
    what they accumulate"""
    import torch
    mpc_gpu, _ = mg
    from mpc_gpu import _lib
    B, G = 9, 64
    dev = torch.device("cuda:0")
    x0, goal, obst = random_batch(B, no, seed=300 + no)
    SENT = -1234.5

    def banded(n, dtype=torch.float64, fill=0.0):
        a = torch.full((n + 2 * G,), SENT if dtype == torch.float64 else -77, dtype=dtype, device=dev)
        a[G:G + n] = fill
        return a, a[G:G + n]

    def intact(a, n):
        s = SENT if a.dtype == torch.float64 else -77
        return bool((a[:G] == s).all()) and bool((a[G + n:] == s).all())

    with mpc_gpu.BatchedMpc(N, no, 0.1 * N, max_batch=B) as s:
        arrs = {}
        def mk(name, n, dtype=torch.float64, data=None, fill=0.0):
            full, inner = banded(n, dtype, fill)
            if data is not None:
                inner.copy_(torch.from_numpy(np.ascontiguousarray(data).reshape(-1)).to(dev))
            arrs[name] = (full, inner, n)
            return inner
        dx0 = mk("x0", B * 5, data=x0); dgoal = mk("goal", B * 2, data=goal); dobst = mk("obst", B * no * 4, data=obst)
        X = mk("X", B * (N + 1) * 5); U = mk("U", B * N * 2)
        u0 = mk("u0", B * 2); cost = mk("cost", B); status = mk("status", B, torch.int32); iters = mk("iters", B, torch.int32)
        noise = mk("noise", B * no * 2, data=np.random.default_rng(1).standard_normal((B, no, 2)))
        margin = mk("margin", B, fill=float("inf")); flags = mk("flags", B, torch.int32); steps = mk("steps", B, torch.int32)
        iacc = mk("iacc", B, torch.int32); sacc = mk("sacc", B, torch.int32)
        s.set_accumulators(iacc, sacc)
        torch.cuda.synchronize()
        s.reset_guess_dev(B, dx0, X, U)
        fl = (_lib.STEP_SHIFT | _lib.STEP_PLANT | _lib.STEP_OBSTACLES | _lib.STEP_METRICS | _lib.STEP_RESET_ON_FAIL | _lib.STEP_ALIAS_BUG)
        s.closed_loop_step_dev(B, dx0, dobst, dgoal, X, U, u0, cost, status, iters, noise, flags=fl, min_margin=margin, ep_flags=flags, ep_steps=steps)
        torch.cuda.synchronize()
        s.set_accumulators(None, None)
        for name, (full, inner, n) in arrs.items():
            assert intact(full, n), name
        st = status.cpu().numpy(); it = iters.cpu().numpy()
        assert np.array_equal(iacc.cpu().numpy(), it)
        assert np.array_equal(sacc.cpu().numpy(), (st == 4).astype(np.int32) + 65536 * (st == 2).astype(np.int32))
        assert np.isfinite(margin.cpu().numpy()).all() and (steps.cpu().numpy() <= 1).all()
        assert s.kernel_name(B).startswith(f"rti_wide_kernel<{cap_of(no)},")


@pytest.mark.parametrize("scen", ["RANDOM", "EDGE"])
def test_wide_scenarios_equal_the_reference_generator(mg, scen):
    mpc_gpu, _ = mg
    from mpc_gpu import world
    with mpc_gpu.BatchedMpc(20, 30, 2.0, max_batch=64) as s:
        got = s.generate_scenarios(scen, 64)
    for sd in range(64):
        obs = world.generate_random_moving_obstacles(scen, n_obst=30, rng=np.random.RandomState(sd))
        ref = world.obstacle_states(obs)
        assert np.array_equal(got[sd], ref), sd


def test_run_grid_writes_the_reference_files(mg, tmp_path):
    mpc_gpu, _ = mg
    cells = mpc_gpu.run_grid(TF=(1, 2), N_OBST=(15, 30), seeds=8, max_iter=60, out_dir=str(tmp_path))
    assert len(cells) == 2 * 2 * 2
    csvs = sorted(glob.glob(os.path.join(tmp_path, "*_experiment_data.csv")))
    specs = sorted(glob.glob(os.path.join(tmp_path, "*_experiment_spec.json")))
    assert len(csvs) == 8 and len(specs) == 8
    for c in cells:
        sp = json.load(open(os.path.join(tmp_path, c["stamp"] + "_experiment_spec.json")))
        assert set(sp) == {"slack", "random_move", "init_guess", "scenario", "TF", "N_SOLV", "N_OBST", "QP_ITER"}
        assert sp["N_SOLV"] == int(sp["TF"] * 10)
        tb = np.loadtxt(os.path.join(tmp_path, c["stamp"] + "_experiment_data.csv"), delimiter=";")
        assert tb.shape == (8, 6)
        x0 = np.tile([-7.0, -7.0, np.pi / 4, 0, 0], (8, 1)); goal = np.tile([7.0, 7.0], (8, 1))
        r = mpc_gpu.run_episodes(x0, goal, sp["scenario"], N=sp["N_SOLV"], Tf=float(sp["TF"]), max_iter=60, random_move=True,
                                 init_guess_when_error=True, n_obst=sp["N_OBST"], first_seed=0, qp_iter_max=sp["QP_ITER"])
        assert np.array_equal(r["table"], c["table"])
        assert np.allclose(tb, c["table"], rtol=1e-15, atol=0)


def test_wide_errors(mg):
    mpc_gpu, _ = mg
    with pytest.raises(mpc_gpu.MpcError, match="N <= 31"):
        mpc_gpu.BatchedMpc(40, 15, 4.0, max_batch=4)
    with mpc_gpu.BatchedMpc(20, 15, 2.0, max_batch=4) as s:
        s.set_lanes_per_stage(3)
        x0, goal, obst = random_batch(4, 15, seed=3)
        with pytest.raises(mpc_gpu.MpcError, match="two lanes per horizon stage"):
            s.solve(x0, obst, goal)
