"""What several SQP iterations per launch (mpc_set_sqp) cost and give, on the GPU.

Timing, per cell and K in (2, 3): the same seeded batch runs `--steps` control steps of K iterations each in three forms on ONE handle --
  "fused":   set_sqp(K, 0): ONE launch per control step (mpc_closed_loop_step_dev on the level-5 kernel; step_tol = 0, so every instance runs all K);
  "host_l0": K launches per control step on the level-0 kernel: K - 1 plain solves (the fused entry point without a step flag: look-ahead and solve) and
             the fused step behind them -- what a caller had to do before;
  "host_l4": the same K launches on the level-4 kernel (the handle's own bounds through mpc_set_instance_bounds_dev), the instantiation level 5 is built on.
The three forms solve the same problems (same_final_state compares the plant states bit for bit).  Beside them "l4_single" and "l5_single" run ONE
iteration per control step on the level-4 kernel and on the level-5 kernel (set_sqp(2, inf)): the cost of one iteration on either.  Each rep restarts
from the same state; timed on the step's stream by scripts/measure.py's protocol (HIP event window, rep 0 a warm-up of every form, the forms alternating
rep by rep).

Rates: for K = 1, 2, 3 the episode harness over the RANDOM scenario (run_episodes, seeds 0 .. --episodes - 1, the reference's experiment: TF = 2,
N = 20, 5 obstacles, QP_ITER = 100): reached and hit rates and the mean step count.

    python scripts/sqp_rate.py [--cell C2] [--reps 5] [--steps 20] [--episodes 2000] [--no-rates] [--out profiles/sqp_rates.json]
"""
import argparse
import json
import os

import numpy as np

import measure

CELLS = [("C2", 1024, 20, 3), ("N50x4096", 4096, 50, 10)]
KS = (2, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell", choices=[c[0] for c in CELLS], action="append")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--episodes", type=int, default=2000)
    ap.add_argument("--no-rates", action="store_true")
    ap.add_argument("--out", default=os.path.join(measure.ROOT, "profiles", "sqp_rates.json"))
    a = ap.parse_args()
    torch = measure.require_gpu()
    import mpc_gpu
    from helpers import random_batch
    L = mpc_gpu._lib
    dev = torch.device("cuda", 0)
    STEP = L.STEP_SHIFT | L.STEP_PLANT | L.STEP_OBSTACLES
    rows = []
    for name, B, N, no in CELLS:
        if a.cell and name not in a.cell:
            continue
        x0, goal, obst = random_batch(B, no, seed=2024 + B + N)
        x0[:, 3:] = 0.0
        with mpc_gpu.BatchedMpc(N, no, 0.1 * N, max_batch=B) as s, measure.own_stream(torch) as st:
            cs = st.cuda_stream
            tx0, to0, tg = (torch.tensor(v, device=dev) for v in (x0, obst, goal))
            tx, to = tx0.clone(), to0.clone()
            X = torch.zeros((B, N + 1, 5), dtype=torch.float64, device=dev); U = torch.zeros((B, N, 2), dtype=torch.float64, device=dev)
            u0 = torch.zeros((B, 2), dtype=torch.float64, device=dev)
            status = torch.zeros(B, dtype=torch.int32, device=dev); iters = torch.zeros(B, dtype=torch.int32, device=dev)
            table = torch.tensor(mpc_gpu.pack_instance_bounds(s.cfg, B), device=dev)
            # form -> (SQP setting, bounds table, launches per control step)
            forms = {"l4_single": ((1, 0.0), table, 1), "l5_single": ((2, float("inf")), None, 1)}
            for K in KS:
                forms[f"fused_K{K}"] = ((K, 0.0), None, 1)
                forms[f"host_l0_K{K}"] = ((1, 0.0), None, K)
                forms[f"host_l4_K{K}"] = ((1, 0.0), table, K)
            names, last = {}, {}

            def rep(form, sqp, tab, launches):      # milliseconds per control step
                def prepare():
                    s.set_instance_bounds_dev(tab)
                    s.set_sqp(*sqp)
                    names[form] = s.kernel_name(B)
                    tx.copy_(tx0); to.copy_(to0)
                    s.reset_guess_dev(B, tx, X, U, stream=cs)

                def step():
                    for _ in range(launches - 1):
                        s.closed_loop_step_dev(B, tx, to, tg, X, U, u0, None, status, iters, flags=0, stream=cs)
                    s.closed_loop_step_dev(B, tx, to, tg, X, U, u0, None, status, iters, flags=STEP, stream=cs)
                ms = measure.window(torch, st, step, a.steps, prepare)
                last[form] = tx.clone()
                return ms

            times = measure.alternate({f: (lambda f=f, v=v: rep(f, *v)) for f, v in forms.items()}, a.reps)
            s.set_instance_bounds_dev(None); s.set_sqp()
            res = {}
            for form, (sqp, tab, launches) in forms.items():
                ms, spread = measure.summary(times[form])
                res[form] = dict(kernel=names[form], launches_per_step=launches, ms_per_control_step=ms, spread=spread)
            for K in KS:
                f = res[f"fused_K{K}"]["ms_per_control_step"]
                res[f"K{K}"] = dict(fused_over_host_l0=f / res[f"host_l0_K{K}"]["ms_per_control_step"], fused_over_host_l4=f / res[f"host_l4_K{K}"]["ms_per_control_step"],
                                    fused_ms_per_iteration=f / K, l4_single_ms=res["l4_single"]["ms_per_control_step"], l5_single_ms=res["l5_single"]["ms_per_control_step"],
                                    same_final_state=bool(torch.equal(last[f"fused_K{K}"], last[f"host_l0_K{K}"]) and torch.equal(last[f"fused_K{K}"], last[f"host_l4_K{K}"])))
        rows.append(dict(cell=name, batch=B, N=N, n_obst=no, **res))
        print(json.dumps(rows[-1]), flush=True)
    rates = None
    if not a.no_rates:
        E = a.episodes
        x0 = np.tile([-7.0, -7.0, np.pi / 4, 0, 0], (E, 1)); goal = np.tile([7.0, 7.0], (E, 1))
        rates = dict(scenario="RANDOM", episodes=E, N=20, Tf=2.0, n_obst=5, qp_iter_max=100, step_tol=0.0, per_K={})
        for K in (1, 2, 3):
            tb = mpc_gpu.run_episodes(x0, goal, "RANDOM", N=20, Tf=2.0, max_iter=400, first_seed=0, qp_iter_max=100, sqp=(K, 0.0))["table"]
            rates["per_K"][str(K)] = dict(reached=float(tb[:, 1].mean()), hit=float(tb[:, 0].mean()), out_of_bounds=float(tb[:, 5].mean()), mean_steps=float(tb[:, 4].mean()))
            print(json.dumps({f"rates_K{K}": rates["per_K"][str(K)]}), flush=True)
    measure.merge_cells(a.out, dict(reps=a.reps, steps_per_rep=a.steps), rows, [c[0] for c in CELLS], extra=dict(rates=rates))      # --no-rates keeps the file's


if __name__ == "__main__":
    main()
