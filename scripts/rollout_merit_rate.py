"""What the rollout merit costs and what it buys (mpc_rollout_merit_dev, MultiStartMpc(select_by="rollout"); DESIGN.md sections 4l and 5i).  The method is
scripts/multistart_rate.py's (section 5h): HIP events around `--launches` back-to-back launches on the object's stream, `--reps` times after one warm-up
rep, median and spread ((max - min) / median).

(a) LAUNCH TIMES at section 5h(a)'s two shapes (G = 1024 and 13107 scenarios x K = 5 members, N = 20, 3 obstacles): mpc_predict_dev on the G scenario rows,
    mpc_rollout_merit_dev on the G K members (merit, defect and margin, members = K), and both together, as shares of the solve launch -- the unchanged solve
    of the parent commit, taken as (seed + solve) - seed as in 5h(a).
(b) CLOSED-LOOP OUTCOME, recorded and not asserted: section 5h(b)'s protocol and its four rows (select_by="cost") run again, and beside them
    select_by="rollout" at incumbent margins 0, 0.1 and 0.5.
(c) bench.py --gpus 1 --steps 20 --warmup 5 with the parent commit's library (`--parent-lib PATH`, handed to the run as MPC_GPU_LIB) and this one's,
    alternating `--bench-rounds` times (--this-first: the other order, to tell a difference between the libraries from one between first and second run
    of a pair); without --parent-lib the part is skipped.
--part a / b / c run one part; the JSON is merged part by part.

    python scripts/rollout_merit_rate.py [--part a] [--part b] [--part c --parent-lib PATH] [--out profiles/rollout_merit_rates.json]
"""
import argparse
import json
import os

import numpy as np

import measure

GROUPS = (1024, 13107)      # x K = 5: 5120 and 65535 instances
N, NO, TF = 20, 3, 2.0


def launch_times(a, torch, mpc_gpu):
    from helpers import random_batch
    rows = []
    for G in GROUPS:
        x0, goal, obst = random_batch(G, NO, seed=4242 + G)
        x0[:, 3:] = 0.0
        with mpc_gpu.MultiStartMpc(N, NO, TF, scenarios=G, select_by="rollout") as ms:
            K, B, m = ms.K, ms.B, ms.inner
            with measure.own_stream(torch, ms.stream) as st:
                cs = st.cuda_stream
                ms._load(x0, obst, goal)
                x_rows, goal_rows, obst_rows = ms._x0[:, 0].contiguous(), ms._goal[:, 0].contiguous(), ms._obst[:, 0].contiguous()

                def seed():
                    ms._seed(x_rows, goal_rows, False, cs)

                def solve():
                    m.closed_loop_step_dev(B, ms._x0, ms._obst, ms._goal, ms.X, ms.U, ms.cand_u0, ms.cand_cost, ms.cand_status, ms.cand_iters, flags=0, stream=cs)

                def predict():
                    m.predict_dev(G, obst_rows, ms._P, stream=cs)

                def merit():
                    m.rollout_merit_dev(B, x_rows, ms._P, goal_rows, ms.U, X=ms.X, merit=ms.cand_merit, defect=ms.cand_defect, margin=ms.cand_margin, members=K, stream=cs)

                def us(body, prepare=None):      # microseconds per pass
                    return lambda: 1e3 * measure.window(torch, st, body, a.launches, prepare)

                seed_solve = lambda: (seed(), solve())
                # in front of the rollout's windows one solve from the guesses: the iterates they read
                t = measure.alternate(dict(seed=us(seed), seed_solve=us(seed_solve), predict=us(predict, seed_solve), merit=us(merit),
                                           predict_merit=us(lambda: (predict(), merit()))), a.reps)
                torch.cuda.synchronize()
                kernel = m.kernel_name(B)
                merits, costs, status = ms.cand_merit.cpu().numpy(), ms.cand_cost.cpu().numpy(), ms.cand_status.cpu().numpy()
                defect = ms.cand_defect.cpu().numpy()
            med, spread = measure.summaries(t)
            solve_us = med["seed_solve"] - med["seed"]
            # what the merit launch must move: U and X read, P read once per group, x0 / goal; three doubles written per instance
            moved = B * 8 * (2 * N + 5 * (N + 1) + 3) + G * 8 * ((N + 1) * NO * 2 + 7)
            ok = ((status == 0) | (status == 2)) & np.isfinite(merits)
            by_cost = np.where(ok, costs, np.inf).reshape(G, K).argmin(axis=1)
            by_merit = np.where(ok, merits, np.inf).reshape(G, K).argmin(axis=1)
            rows.append(dict(groups=G, K=K, instances=B, N=N, n_obst=NO, solve_kernel=kernel,
                             us=dict(solve=solve_us, predict=med["predict"], merit=med["merit"], predict_merit=med["predict_merit"]), spread=spread,
                             predict_over_solve=med["predict"] / solve_us, merit_over_solve=med["merit"] / solve_us,
                             predict_merit_over_solve=med["predict_merit"] / solve_us, merit_bytes=moved, merit_GBps=moved / med["merit"] / 1e3,
                             argmins_differ=float((by_cost != by_merit).mean()), defect_median=float(np.median(defect)),
                             merit_over_cost_median=float(np.median(merits[ok] / costs[ok]))))
            print(json.dumps(rows[-1]), flush=True)
    return dict(reps=a.reps, launches_per_rep=a.launches, cells=rows)


def closed_loop(a, torch, mpc_gpu):
    from mpc_gpu.experiments import GOAL, START
    from mpc_gpu import world as w
    seeds, max_iter, no = 100, 400, w.N_OBST
    r_hit = w.R_OBST + w.R_ROBOT
    out = []
    five = mpc_gpu.multistart.DEFAULT_OFFSETS
    rows = [((0.0,), 0.0, "cost"), (five, 0.0, "cost"), (five, 0.1, "cost"), (five, 0.5, "cost"), (five, 0.0, "rollout"), (five, 0.1, "rollout"), (five, 0.5, "rollout")]
    for offsets, m_inc, by in rows:
        with mpc_gpu.MultiStartMpc(w.N_SOLV, no, w.TF, scenarios=seeds, offsets=offsets, incumbent_margin=m_inc, select_by=by) as ms:
            dev, m = ms.dev, ms.inner
            with torch.cuda.stream(ms.stream):
                cs = ms.stream.cuda_stream
                x = torch.tensor(np.tile(START, (seeds, 1)), dtype=torch.float64, device=dev)
                goal = torch.tensor(np.tile(GOAL, (seeds, 1)), dtype=torch.float64, device=dev)
                obst = torch.zeros(seeds, no, 4, dtype=torch.float64, device=dev)
                m.generate_scenarios_dev("RANDOM", seeds, obst, seed0=0, stream=cs)
                state = m.noise_state(seeds, "RANDOM", seed0=0, stream=cs)
                noise = torch.zeros(seeds, no, 2, dtype=torch.float64, device=dev)
                reached = torch.zeros(seeds, dtype=torch.bool, device=dev)
                steps = torch.zeros(seeds, dtype=torch.int32, device=dev)
                margin = torch.full((seeds,), float("inf"), dtype=torch.float64, device=dev)
                lost = torch.zeros(seeds, dtype=torch.int32, device=dev)
                switched = torch.zeros(seeds, dtype=torch.int32, device=dev)
                for k in range(max_iter):
                    m.noise_draw_dev(seeds, state, noise, stream=cs)
                    res = ms.step(x, obst, goal, noise=noise, randomness=w.RANDOMNESS, vmax=w.V_MAX_OBST)
                    live = ~reached
                    d = torch.linalg.norm(x[:, None, :2] - obst[:, :, :2], dim=2).min(dim=1).values - r_hit
                    margin = torch.where(live, torch.minimum(margin, d), margin)
                    lost += (live & (res["winner"] < 0)).int()
                    switched += (live & (res["winner"] > 0)).int()
                    now = torch.linalg.norm(x[:, :2] - goal, dim=1) <= w.TOL
                    steps += (live & ~now).int()
                    reached |= now
                    if k % 25 == 24 and bool(reached.all()):
                        break
                torch.cuda.synchronize()
            reached, steps, margin = reached.cpu().numpy(), steps.cpu().numpy(), margin.cpu().numpy()
            out.append(dict(K=len(offsets), offsets=list(offsets), incumbent_margin=m_inc, select_by=by, seeds=seeds, max_iter=max_iter, N=w.N_SOLV, n_obst=no,
                            reached=int(reached.sum()), hit=int((margin <= 0).sum()), reached_without_hit=int((reached & (margin > 0)).sum()),
                            mean_steps_of_reached=float(steps[reached].mean()) if reached.any() else None, min_margin_median=float(np.median(margin)),
                            steps_without_winner=int(lost.cpu().numpy().sum()), steps_won_by_another_member=int(switched.cpu().numpy().sum())))
            print(json.dumps(out[-1]), flush=True)
    return dict(runs=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["a", "b", "c"], action="append")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--this-first", action="store_true", help="part c: this commit's library runs first in every round (recorded as bench_this_first)")
    ap.add_argument("--out", default=os.path.join(measure.ROOT, "profiles", "rollout_merit_rates.json"))
    a = ap.parse_args()
    parts = a.part or (["a", "b"] + (["c"] if a.parent_lib else []))
    res = measure.read_json(a.out)
    if "a" in parts or "b" in parts:
        torch = measure.require_gpu()
        import mpc_gpu
        if "a" in parts:
            res["launch_times"] = launch_times(a, torch, mpc_gpu)
        if "b" in parts:
            res["closed_loop"] = closed_loop(a, torch, mpc_gpu)
    if "c" in parts:
        res["bench_this_first" if a.this_first else "bench"] = measure.bench_ab(a.parent_lib, a.bench_rounds, a.this_first)
    measure.write_json(a.out, res)


if __name__ == "__main__":
    main()
