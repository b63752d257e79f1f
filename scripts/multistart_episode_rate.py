"""What the group control step costs and what multi-start buys at the reference's 1000 seeds (mpc_group_step_dev, MultiStartMpc.step_fused,
run_multistart_episodes; DESIGN.md sections 4m and 5j).  The method is scripts/multistart_rate.py's: HIP events on the object's stream, one warm-up rep, median
and spread (max - min over median) of `--reps` reps.

(a) TIME OF ONE CONTROL STEP for G scenarios of K = 5 members (N = 20, 3 obstacles, random scenarios of tests/helpers.random_batch), `--launches` consecutive
    control steps per rep from the same start (restart() and the same states in front of every rep):
      composed   MultiStartMpc.step, the parent commit's control step (its Python is unchanged): the yardstick;
      fused      MultiStartMpc.step_fused: member solve + mpc_group_step_dev;
      solve      the solve launch alone on the members (closed_loop_step_dev, flags = 0): the floor;
      tail       mpc_group_step_dev alone on what a solve left, with the bytes it must move over its time.
(b) CLOSED-LOOP OUTCOME at the reference's 1000 seeds, recorded and not asserted: section 5h(b)'s four rows (K = 1; K = 5 with incumbent_margin 0, 0.1, 0.5)
    through run_multistart_episodes (start [-7, -7, pi/4, 0, 0], goal [7, 7], RANDOM, 5 obstacles, the reference's noise stream, 400 steps at most), and
    select_by="rollout" for the two margin rows.
(c) bench.py --gpus 1 --steps 20 --warmup 5 with the parent commit's library (`--parent-lib PATH`) and this one's, alternating (scripts/measure.py's
    bench_ab): the flagship path launches nothing of this change.
(d) the largest difference between the fused tail and the composition over the lockstep shapes of tests/test_gpu_multistart_episodes.py.

    python scripts/multistart_episode_rate.py [--part a] [--part b] [--part c --parent-lib PATH] [--part d] [--out profiles/multistart_episode_rates.json]
"""
import argparse
import json
import os
import time

import numpy as np

import measure

GROUPS = (1024, 13107)      # x K = 5: 5120 and 65535 instances
N, NO, TF = 20, 3, 2.0


def step_times(a, torch, mpc_gpu):
    from helpers import random_batch
    L = mpc_gpu._lib
    rows = []
    for G in GROUPS:
        x0, goal, obst0 = random_batch(G, NO, seed=4242 + G)
        x0[:, 3:] = 0.0
        with mpc_gpu.MultiStartMpc(N, NO, TF, scenarios=G) as ms:
            K, B = ms.K, ms.B
            with measure.own_stream(torch, ms.stream) as st:
                cs = st.cuda_stream
                up = lambda h: torch.from_numpy(np.ascontiguousarray(h)).to(ms.dev)
                x_init, o_init, dgoal = up(x0), up(obst0), up(goal)
                x, ob = x_init.clone(), o_init.clone()

                def start():
                    ms.restart()
                    x.copy_(x_init); ob.copy_(o_init)

                def us(body, prepare):      # microseconds per control step
                    return lambda: 1e3 * measure.window(torch, st, body, a.launches, prepare)

                def solve():
                    ms.inner.closed_loop_step_dev(B, ms._x0, ms._obst, ms._goal, ms.X, ms.U, ms.cand_u0, ms.cand_cost, ms.cand_status, ms.cand_iters, flags=0, stream=cs)

                def tail():
                    L.check(L.lib().mpc_group_step_dev(ms.inner._h, G, K, ms.cand_cost.data_ptr(), ms.cand_status.data_ptr(), ms.cand_u0.data_ptr(), 0.0, 0,
                                                       x.data_ptr(), ob.data_ptr(), dgoal.data_ptr(), ms.offsets.data_ptr(), None, 0.1, 2.0,
                                                       ms.X.data_ptr(), ms.U.data_ptr(), ms._out, cs))

                def prepare_solved():      # the members loaded and seeded, one solve behind them: what the floor and the tail work on
                    start()
                    ms.step_fused(x, ob, dgoal)

                t = measure.alternate(dict(composed=us(lambda: ms.step(x, ob, dgoal), start), fused=us(lambda: ms.step_fused(x, ob, dgoal), start),
                                           solve=us(solve, prepare_solved), tail=us(tail, prepare_solved)), a.reps)
                idle = int((ms.ep_flags & 1).sum().item())
                kernel = ms.inner.kernel_name(B)
            med, spread = measure.summaries(t)
            row_bytes = 8 * (5 * (N + 1) + 2 * N)
            # read: the winner's row, K (key, status), the u0 row, x, goal, obstacles, bookkeeping; written: K rows, x, obstacles, the members' inputs, bookkeeping
            moved = G * (row_bytes + K * 12 + 16 + 40 + 16 + NO * 32 + 24 + K * row_bytes + 40 + NO * 32 + K * (40 + NO * 32 + 16 + 4) + 44)
            rows.append(dict(groups=G, K=K, instances=B, N=N, n_obst=NO, solve_kernel=kernel, steps_per_rep=a.launches, us=med, spread=spread,
                             fused_over_composed=med["fused"] / med["composed"], composed_over_solve=med["composed"] / med["solve"],
                             fused_over_solve=med["fused"] / med["solve"], tail_over_solve=med["tail"] / med["solve"], tail_bytes=moved,
                             tail_GBps=moved / med["tail"] / 1e3, groups_idle_at_the_end=idle))
            print(json.dumps(rows[-1]), flush=True)
    return dict(reps=a.reps, steps_per_rep=a.launches, cells=rows)


def closed_loop(a, torch, mpc_gpu):
    from mpc_gpu.experiments import GOAL, START
    from mpc_gpu import world as w
    five = mpc_gpu.multistart.DEFAULT_OFFSETS
    out = []
    for offsets, m_inc, by in (((0.0,), 0.0, "cost"), (five, 0.0, "cost"), (five, 0.1, "cost"), (five, 0.5, "cost"), (five, 0.1, "rollout"), (five, 0.5, "rollout")):
        t0 = time.perf_counter()
        r = mpc_gpu.run_multistart_episodes(np.tile(START, (a.seeds, 1)), GOAL, "RANDOM", offsets=offsets, incumbent_margin=m_inc, select_by=by, N=w.N_SOLV, Tf=w.TF,
                                            n_obst=w.N_OBST, max_iter=400, first_seed=0)
        wall = time.perf_counter() - t0
        tb = r["table"]
        reached, hit = tb[:, 1] == 1, tb[:, 0] == 1
        out.append(dict(K=len(offsets), offsets=list(offsets), incumbent_margin=m_inc, select_by=by, seeds=a.seeds, max_iter=400, N=w.N_SOLV, n_obst=w.N_OBST,
                        reached=int(reached.sum()), hit=int(hit.sum()), reached_without_hit=int((reached & ~hit).sum()), out_of_bounds=int(tb[:, 5].sum()),
                        mean_steps_of_reached=float(tb[reached, 4].mean()) if reached.any() else None, min_margin_median=float(np.median(tb[:, 2])),
                        steps_without_winner=int(r["lost_steps"].sum()), steps_won_by_another_member=int(r["switched_steps"].sum()), steps_run=r["steps_run"],
                        member_solves=r["solves"], wall_s=wall))
        print(json.dumps(out[-1]), flush=True)
    return dict(runs=out)


def lockstep_difference(a, torch, mpc_gpu):
    import multistart_episode_cases as ec
    import test_gpu_multistart_episodes as tg
    from feature_loop import on_own_stream
    worst = {}
    for shape, name in zip(ec.SHAPES, ec.SHAPE_IDS):
        on_own_stream(lambda s=shape, n=name: worst.__setitem__(n, tg.lockstep(mpc_gpu, s)))
    return dict(tolerance=tg.TOL, steps=ec.STEPS, largest_difference=worst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["a", "b", "c", "d"], action="append")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--seeds", type=int, default=1000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--this-first", action="store_true")
    ap.add_argument("--out", default=os.path.join(measure.ROOT, "profiles", "multistart_episode_rates.json"))
    a = ap.parse_args()
    parts = a.part or (["a", "b", "d"] + (["c"] if a.parent_lib else []))
    res = measure.read_json(a.out)
    if set(parts) & {"a", "b", "d"}:
        torch = measure.require_gpu()
        import mpc_gpu
        for part, name, fn in (("a", "step_times", step_times), ("b", "closed_loop", closed_loop), ("d", "lockstep", lockstep_difference)):
            if part in parts:
                res[name] = fn(a, torch, mpc_gpu)
    if "c" in parts:
        res["bench"] = measure.bench_ab(a.parent_lib, a.bench_rounds, a.this_first)
    measure.write_json(a.out, res)


if __name__ == "__main__":
    main()
