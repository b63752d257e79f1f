"""The factor sweep's packed LDS requests on the dense split kernels (factor_sweep_requests_cases.py; rowpar_factor<.., PACKED>, rti_kernel.hpp): row 4 of
W~_t fetched from the dead row 5 of the stage's H~aug block, K~ and the factors 1/d0, l, 1/d1 stored by one request (the factors from two mirror lanes).
  1. three solves per row from DYNAMICALLY INCONSISTENT starts (noise 0.2 on X: the affine entry that travels with the relocated row is non-zero in every
     stage) against the oracle, judged as test_gpu_factor_sweep_live_rows.py judges its rows -- N = 2, 3, 20 on three lanes per stage, N = 21 on two;
  2. ten fused control steps at N = 20 / 3 obstacles against helpers.OracleLoop, re-seeded with the GPU's state before every step as in
     test_gpu_off_default.test_fused_step_against_the_oracle_loop (same tolerances): the relocated factor words feed the corrector's k and, through the
     shift, the next step's warm start;
  3. the two-wavefront build (compact blocks: it keeps the sweep's old requests) against the dense kernel, bit for bit, from the same inconsistent starts.
The oracle alone converges on every instance of every row (test_factor_sweep_requests_host.py)."""
import numpy as np
import pytest

import factor_sweep_live_rows_cases as lc
import factor_sweep_requests_cases as rc
import off_default_cases as oc
from feature_loop import GpuLoop, mg
from helpers import OracleLoop, adjudicate, oracle_P, random_batch
from test_gpu_factor_sweep_live_rows import gpu_three_warm_solves
from test_gpu_off_default import judge_solves

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rid", [r["id"] for r in rc.ROWS])
def test_three_solves_from_inconsistent_starts_against_the_oracle(mg, rid):
    mpc_gpu, orc = mg
    row = rc.ROW[rid]
    N, no, B, Tf = row["N"], row["no"], row["B"], row["Tf"]
    x0, goal, obst = rc.batch(row)
    cfg = orc.config(N, no, Tf)
    P = oracle_P(orc, cfg, obst)
    ref = lc.oracle_three_solves(orc, cfg, row, x0, P, goal)
    with mpc_gpu.BatchedMpc(N, no, Tf, max_batch=B) as s:
        name = oc.configure(s, row)
        assert name == row["name"], (rid, name)
        names = [s.kernel_name(B, lookahead=k != 1) for k in range(3)]
        outs = gpu_three_warm_solves(s, ref, x0, obst, P, goal)
    assert names == [row["name"]] * 3, (rid, names)
    judge_solves(orc, cfg, ref, outs, x0, P, goal, row["ok"], False, f"requests {rid} {name} noise {lc.NOISE}")


def test_ten_fused_steps_against_the_oracle_loop(mg):
    mpc_gpu, orc = mg
    c = rc.LOOP
    N, no, B, Tf, K = c["N"], c["no"], c["B"], c["Tf"], c["steps"]
    x0, goal, obst = random_batch(B, no, seed=c["seed"])
    noise = np.random.default_rng(c["noise_seed"]).standard_normal((K, B, no, 2))
    cfg = orc.config(N, no, Tf)
    g = GpuLoop(mpc_gpu, N, no, Tf, x0, goal, obst, alias=False)
    name = g.m.kernel_name(B)
    assert name == c["name"], name
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
                continue
            n_cmp += 1
            assert after["status"][b] == r["status"], (k, b, after["status"][b], r["status"])
            assert np.array_equal(after["obst"][b], L.obst), (k, b)
            assert after["flags"][b] == L.flags and after["steps"][b] == L.steps, (k, b, after["flags"][b], L.flags)
            if r["status"] != 0:
                continue
            d = max(np.abs(after["X"][b] - L.X).max(), np.abs(after["U"][b] - L.U).max())
            if d > 1e-6:                                            # adjudicated against the exact solution of the QP
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
    g.close()
    print(f"REQUESTS fused {name}: compared {n_cmp} adjudicated {n_out} worst {worst}")
    assert n_cmp > 0.7 * B * K and n_out <= max(2, 0.002 * n_cmp), (n_cmp, n_out)
    assert worst["X"] <= 1e-6 and worst["u"] <= 8e-6 and worst["x"] <= 1e-6 and worst["margin"] <= 1e-6, worst


def test_two_wavefront_build_equals_the_dense_kernel_bit_for_bit(mg):
    mpc_gpu, orc = mg
    c = rc.W2
    N, no, B, Tf = c["N"], c["no"], c["B"], c["Tf"]
    x0, goal, obst = random_batch(B, no, seed=c["seed"])
    cfg = orc.config(N, no, Tf)
    P = oracle_P(orc, cfg, obst)
    row = dict(seed=c["seed"])
    res = {}
    for w in (1, 2):
        with mpc_gpu.BatchedMpc(N, no, Tf, max_batch=B) as s:
            s.set_lanes_per_stage(3); s.set_waves_per_simd(w)
            assert s.kernel_name(B) == (c["dense"] if w == 1 else c["w2"]), (w, s.kernel_name(B))
            s.reset_guess(x0)
            outs = []
            for k in range(3):
                X, U = s.get_traj(B)
                s.set_warmstart(lc.perturbed(row, k, X), U)              # the same inconsistent start on both handles: X is equal bit for bit so far
                g = s.solve(x0, obst if k != 1 else P, goal); Xs, Us = s.get_traj(B); s.shift(B)
                outs.append((g, Xs, Us))
            res[w] = outs
    for k, ((ga, Xa, Ua), (gb, Xb, Ub)) in enumerate(zip(res[1], res[2])):
        assert np.array_equal(Xa, Xb) and np.array_equal(Ua, Ub), k
        for key in ("u0", "cost", "status", "iters"):
            assert np.array_equal(ga[key], gb[key]), (k, key)
