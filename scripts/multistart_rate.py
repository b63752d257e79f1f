"""What multi-start solves cost and what they buy (mpc_seed_guesses_dev, mpc_select_best_dev, mpc_gpu.MultiStartMpc; DESIGN.md sections 4k and 5h).

(a) LAUNCH TIMES.  For G scenarios of K = 5 members (N = 20, 3 obstacles, random scenarios of tests/helpers.random_batch) the three launches of one group
    solve, each timed by scripts/measure.py's protocol: `--launches` back-to-back launches between two HIP events on the object's stream, `--reps` times
    after one warm-up rep:
      seed          mpc_seed_guesses_dev alone;
      seed + solve  the guess launch and the ordinary solve launch (closed_loop_step_dev with flags = 0) of the same G K instances -- every solve then
                    starts from the same iterates and does the same work; solve = (seed + solve) - seed is the yardstick, the parent commit's code;
      select        mpc_select_best_dev with MPC_SELECT_BROADCAST on the costs that solve left (from the second launch on it copies what is there
                    already: the same traffic).
    Reported: median time per launch, spread (max - min over median), the ratios to the solve, and for the selection the bytes it must move (the
    winner's rows read once, K - 1 rows written, cost and status read) over its time.
(b) CLOSED-LOOP OUTCOME, recorded and not asserted: the reference's protocol (start [-7, -7, pi/4, 0, 0], goal [7, 7], scenario RANDOM, seeds 0 .. 99,
    noisy obstacles from the reference's own noise stream, at most 400 control steps) through MultiStartMpc.step with K = 1 (offsets (0,): the straight
    guess alone) and K = 5 (the default offsets; incumbent_margin 0, 0.1 and 0.5): goals reached, robots hit (margin to an obstacle's 1.2 m <= 0 before
    the goal), mean steps of those that reached, and the group steps on which no member was eligible.
--part a / --part b run one part (a caller that wants each under a time limit of its own starts one process per part); the JSON is merged part by part.

    python scripts/multistart_rate.py [--part a] [--part b] [--reps 5] [--launches 20] [--out profiles/multistart_rates.json]
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
    L = mpc_gpu._lib
    rows = []
    for G in GROUPS:
        x0, goal, obst = random_batch(G, NO, seed=4242 + G)
        x0[:, 3:] = 0.0
        with mpc_gpu.MultiStartMpc(N, NO, TF, scenarios=G) as ms:
            K, B = ms.K, ms.B
            with measure.own_stream(torch, ms.stream) as st:
                cs = st.cuda_stream
                ms._load(x0, obst, goal)
                x_rows, goal_rows = ms._x0[:, 0].contiguous(), ms._goal[:, 0].contiguous()

                def seed():
                    ms._seed(x_rows, goal_rows, False, cs)

                def solve():
                    ms.inner.closed_loop_step_dev(B, ms._x0, ms._obst, ms._goal, ms.X, ms.U, ms.cand_u0, ms.cand_cost, ms.cand_status, ms.cand_iters, flags=0, stream=cs)

                def select():
                    L.check(L.lib().mpc_select_best_dev(ms.inner._h, G, K, ms.cand_cost.data_ptr(), ms.cand_status.data_ptr(), 0.0, L.SELECT_BROADCAST,
                                                        ms.X.data_ptr(), ms.U.data_ptr(), ms.winner.data_ptr(), ms.cost.data_ptr(), ms.u0.data_ptr(),
                                                        ms.cand_u0.data_ptr(), cs))

                def us(body, prepare=None):      # microseconds per pass
                    return lambda: 1e3 * measure.window(torch, st, body, a.launches, prepare)

                seed_solve = lambda: (seed(), solve())
                # in front of the selection's window one solve from the guesses: the costs it reads
                t = measure.alternate(dict(seed=us(seed), seed_solve=us(seed_solve), select=us(select, seed_solve)), a.reps)
                torch.cuda.synchronize()
                kernel = ms.inner.kernel_name(B)
                winners = ms.winner.cpu().numpy()
                status = ms.cand_status.cpu().numpy()
            med, spread = measure.summaries(t)
            solve_us = med["seed_solve"] - med["seed"]
            row_bytes = 8 * (5 * (N + 1) + 2 * N)
            moved = G * (K * row_bytes + K * 12 + 4 + 8 + 16 + 16)      # read 1 row + write K - 1 rows; cost + status; winner, best_cost, u0 row, best_u0
            rows.append(dict(groups=G, K=K, instances=B, N=N, n_obst=NO, solve_kernel=kernel, us=dict(seed=med["seed"], solve=solve_us, select=med["select"]),
                             spread=spread, seed_over_solve=med["seed"] / solve_us, select_over_solve=med["select"] / solve_us,
                             both_over_solve=(med["seed"] + med["select"]) / solve_us, select_bytes=moved, select_GBps=moved / med["select"] / 1e3,
                             winners_not_member_0=float((winners > 0).mean()), groups_without_winner=int((winners < 0).sum()),
                             status_counts={str(s): int((status == s).sum()) for s in (0, 2, 4)}))
            print(json.dumps(rows[-1]), flush=True)
    return dict(reps=a.reps, launches_per_rep=a.launches, cells=rows)


def closed_loop(a, torch, mpc_gpu):
    from mpc_gpu.experiments import GOAL, START
    from mpc_gpu import world as w
    seeds, max_iter, no = 100, 400, w.N_OBST
    r_hit = w.R_OBST + w.R_ROBOT
    out = []
    five = mpc_gpu.multistart.DEFAULT_OFFSETS
    for offsets, m_inc in (((0.0,), 0.0), (five, 0.0), (five, 0.1), (five, 0.5)):
        with mpc_gpu.MultiStartMpc(w.N_SOLV, no, w.TF, scenarios=seeds, offsets=offsets, incumbent_margin=m_inc) as ms:
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
                for k in range(max_iter):
                    m.noise_draw_dev(seeds, state, noise, stream=cs)
                    res = ms.step(x, obst, goal, noise=noise, randomness=w.RANDOMNESS, vmax=w.V_MAX_OBST)
                    live = ~reached
                    d = torch.linalg.norm(x[:, None, :2] - obst[:, :, :2], dim=2).min(dim=1).values - r_hit
                    margin = torch.where(live, torch.minimum(margin, d), margin)
                    lost += (live & (res["winner"] < 0)).int()
                    now = torch.linalg.norm(x[:, :2] - goal, dim=1) <= w.TOL
                    steps += (live & ~now).int()
                    reached |= now
                    if k % 25 == 24 and bool(reached.all()):
                        break
                torch.cuda.synchronize()
            reached, steps, margin = reached.cpu().numpy(), steps.cpu().numpy(), margin.cpu().numpy()
            out.append(dict(K=len(offsets), offsets=list(offsets), incumbent_margin=m_inc, seeds=seeds, max_iter=max_iter, N=w.N_SOLV, n_obst=no, reached=int(reached.sum()),
                            hit=int((margin <= 0).sum()), reached_without_hit=int((reached & (margin > 0)).sum()),
                            mean_steps_of_reached=float(steps[reached].mean()) if reached.any() else None,
                            min_margin_median=float(np.median(margin)), steps_without_winner=int(lost.cpu().numpy().sum())))
            print(json.dumps(out[-1]), flush=True)
    return dict(runs=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["a", "b"], action="append")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(measure.ROOT, "profiles", "multistart_rates.json"))
    a = ap.parse_args()
    torch = measure.require_gpu()
    import mpc_gpu
    parts = a.part or ["a", "b"]
    res = measure.read_json(a.out)
    if "a" in parts:
        res["launch_times"] = launch_times(a, torch, mpc_gpu)
    if "b" in parts:
        res["closed_loop"] = closed_loop(a, torch, mpc_gpu)
    measure.write_json(a.out, res)


if __name__ == "__main__":
    main()
