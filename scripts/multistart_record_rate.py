"""What the per-group record costs per control step, and what it shows of one episode that multi-start loses (mpc_group_record_set_dev /
mpc_group_record_dev, MultiStartMpc.group_record_set_dev, run_multistart_episodes(record=); DESIGN.md sections 4p and 5m).  The method is
scripts/multistart_episode_rate.py's, on scripts/measure.py: HIP events on the object's stream, one warm-up rep, median and spread (max - min over median) of
`--reps` reps, the forms alternating rep by rep.

(a) TIME OF ONE CONTROL STEP of run_multistart_episodes (MultiStartMpc.step_fused) in section 5j's configuration -- G scenarios of K = 5 members, N = 20,
    3 obstacles, random scenarios of tests/helpers.random_batch, `--launches` consecutive control steps per rep from the same start (restart(), the same
    states and len = 0 in front of every rep) -- in four forms:
      off         no record attached: what step_fused launched before the record existed;
      all_plans   every group recorded, cand_X kept;
      all         every group recorded, cand_X NULL;
      eight       8 groups recorded, cand_X kept.
    The record is attached to one handle and detached between the forms (so the solve kernel and its iterates are the same in all four).
(b) THE LOSING EPISODE: section 5h(b)'s rows K = 1 and K = 5 with incumbent_margin 0 (start [-7, -7, pi/4, 0, 0], goal [7, 7], RANDOM, seeds 0 .. 99, 5 obstacles,
    the reference's noise stream, 400 steps at most) through run_multistart_episodes, the K = 5 row with record=True; the seeds that reach their goal with one
    start and not with five are listed, and the first of them is summarised step by step (`--seed` picks another): distance to the goal, the winner and its
    changes, and the keys, status words and plans of the candidates step by step where the winner changes most, where most steps have no winner, and at the end.
(c) bench.py --gpus 1 --steps 20 --warmup 5 with the parent commit's library (`--parent-lib PATH`) and this one's, alternating (measure.bench_ab): the
    flagship path launches nothing of this change.

    python scripts/multistart_record_rate.py [--part a] [--part b] [--part c --parent-lib PATH] [--out profiles/multistart_record_rates.json]
"""
import argparse
import json
import os

import numpy as np

import measure

GROUPS = (1024, 13107)      # x K = 5: 5120 and 65535 instances (section 5j)
N, NO, TF = 20, 3, 2.0
FORMS = ("off", "all_plans", "all", "eight")


def step_times(a, torch, mpc_gpu):
    from helpers import random_batch
    from mpc_gpu.multistart import group_record_bytes
    rows = []
    T = a.launches
    for G in GROUPS:
        x0, goal, obst0 = random_batch(G, NO, seed=4242 + G)
        x0[:, 3:] = 0.0
        with mpc_gpu.MultiStartMpc(N, NO, TF, scenarios=G) as ms:
            K, B = ms.K, ms.B
            with measure.own_stream(torch, ms.stream) as st:
                up = lambda h: torch.from_numpy(np.ascontiguousarray(h)).to(ms.dev)
                x_init, o_init, dgoal = up(x0), up(obst0), up(goal)
                x, ob = x_init.clone(), o_init.clone()
                f64 = dict(dtype=torch.float64, device=ms.dev); i32 = dict(dtype=torch.int32, device=ms.dev)

                def arrays(groups, plans):
                    R = len(groups)
                    row = np.full(G, -1, dtype=np.int32); row[groups] = np.arange(R, dtype=np.int32)
                    return dict(group_row=up(row), len=torch.zeros(R, **i32), x=torch.zeros(R, T + 1, 5, **f64), obst=torch.zeros(R, T + 1, NO, 4, **f64),
                                u=torch.zeros(R, T, 2, **f64), winner=torch.zeros(R, T, **i32), best_key=torch.zeros(R, T, **f64), cand_key=torch.zeros(R, T, K, **f64),
                                cand_status=torch.zeros(R, T, K, **i32), cand_iters=torch.zeros(R, T, K, **i32), cand_u0=torch.zeros(R, T, K, 2, **f64),
                                cand_X=torch.zeros(R, T, K, N + 1, 5, **f64) if plans else None)

                every, eight = np.arange(G), np.arange(8) * (G // 8)
                recs = dict(off=None, all_plans=arrays(every, True), all=arrays(every, False), eight=arrays(eight, True))
                nbytes = dict(off=0, all_plans=group_record_bytes(G, T, N, NO, K, True), all=group_record_bytes(G, T, N, NO, K, False),
                              eight=group_record_bytes(8, T, N, NO, K, True))

                def form(name):
                    rec = recs[name]

                    def prepare():
                        ms.restart()
                        x.copy_(x_init); ob.copy_(o_init)
                        if rec is None:
                            ms.group_record_set_dev(0)
                        else:
                            rec["len"].zero_()
                            ms.group_record_set_dev(rec["len"].shape[0], T, **rec)
                    return lambda: 1e3 * measure.window(torch, st, lambda: ms.step_fused(x, ob, dgoal), a.launches, prepare)

                t = measure.alternate({n: form(n) for n in FORMS}, a.reps)
                ms.group_record_set_dev(0)
                recorded = {n: int(recs[n]["len"].sum().item()) for n in FORMS if recs[n] is not None}
                kernel = ms.inner.kernel_name(B)
            med, spread = measure.summaries(t)
            rows.append(dict(groups=G, K=K, instances=B, N=N, n_obst=NO, solve_kernel=kernel, steps_per_rep=a.launches, us=med, spread=spread,
                             over_off={n: med[n] / med["off"] for n in FORMS}, added_us={n: med[n] - med["off"] for n in FORMS}, record_bytes=nbytes,
                             bytes_per_step={n: nbytes[n] / T for n in FORMS}, steps_recorded_in_the_last_rep=recorded))
            print(json.dumps(rows[-1]), flush=True)
    return dict(reps=a.reps, steps_per_rep=a.launches, cells=rows)


def _lateral(plan, x, goal):
    """the largest signed distance of a plan's positions from the line x -> goal (left of it positive)"""
    d = goal - x[:2]
    n = np.array([-d[1], d[0]]) / max(np.linalg.norm(d), 1e-12)
    lat = (plan[:, :2] - x[:2]) @ n
    return float(lat[np.argmax(np.abs(lat))])


def losing_episode(a, torch, mpc_gpu):
    from mpc_gpu.experiments import GOAL, START
    from mpc_gpu import world as w
    five = mpc_gpu.multistart.DEFAULT_OFFSETS
    kw = dict(incumbent_margin=0.0, select_by="cost", N=w.N_SOLV, Tf=w.TF, n_obst=w.N_OBST, max_iter=400, first_seed=0)
    x0 = np.tile(START, (a.seeds, 1))
    one = mpc_gpu.run_multistart_episodes(x0, GOAL, "RANDOM", offsets=(0.0,), **kw)
    many = mpc_gpu.run_multistart_episodes(x0, GOAL, "RANDOM", offsets=five, record=True, **kw)
    plain = mpc_gpu.run_multistart_episodes(x0, GOAL, "RANDOM", offsets=five, **kw)
    assert np.array_equal(plain["table"], many["table"]) and np.array_equal(plain["x_last"], many["x_last"])          # the record changes no row
    r1, r5 = one["table"][:, 1] == 1, many["table"][:, 1] == 1
    lost_by_many = np.nonzero(r1 & ~r5)[0].tolist()
    out = dict(seeds=a.seeds, reached_one=int(r1.sum()), reached_five=int(r5.sum()), reached_by_one_start_alone=lost_by_many,
               reached_by_five_starts_alone=np.nonzero(~r1 & r5)[0].tolist(), record_bytes=mpc_gpu.group_record_bytes(a.seeds, 400, w.N_SOLV, w.N_OBST, 5))
    if not lost_by_many:
        return out
    g = a.seed if a.seed is not None else lost_by_many[0]
    t = many["record"][g]
    L = t["u"].shape[0]
    goal = np.asarray(GOAL, dtype=np.float64)
    dist = np.linalg.norm(t["simX"][:, :2] - goal, axis=1)
    margin = (np.linalg.norm(t["simX"][:, None, :2] - t["obst_traj"][:, :, :2], axis=2) - 1.2).min(axis=1)
    win = t["winner"]
    change = np.concatenate([[False], win[1:] != win[:-1]])
    ok = ((t["cand_status"] == 0) | (t["cand_status"] == 2)) & np.isfinite(t["cand_key"])
    windows = []
    for lo in range(0, L, 25):
        hi = min(lo + 25, L)
        windows.append(dict(steps=[lo, hi], dist_to_goal=[float(dist[lo]), float(dist[hi])], least_margin=float(margin[lo:hi + 1].min()),
                            winner_counts=np.bincount(win[lo:hi] + 1, minlength=6).tolist(), winner_changes=int(change[lo:hi].sum()),
                            eligible_per_member=ok[lo:hi].sum(axis=0).tolist(), speed=float(np.abs(t["simX"][lo:hi, 3]).mean())))
    # step by step: the 25-step window in which the winner changes most, the one with the most steps without a winner, and the last three steps
    def steps(lo, hi):
        return [dict(step=j, state=t["simX"][j].tolist(), dist_to_goal=float(dist[j]), margin=float(margin[j]), winner=int(win[j]), key=float(t["key"][j]),
                     cand_key=[float(v) for v in t["cand_key"][j]], cand_status=t["cand_status"][j].tolist(), cand_iters=t["cand_iters"][j].tolist(),
                     u=t["u"][j].tolist(), plan_lateral=[_lateral(t["cand_X"][j, k], t["simX"][j], goal) for k in range(t["cand_X"].shape[1])],
                     plan_end_dist=[float(np.linalg.norm(t["cand_X"][j, k, -1, :2] - goal)) for k in range(t["cand_X"].shape[1])]) for j in range(lo, hi)]
    changes, lost = max(windows, key=lambda d: d["winner_changes"])["steps"], max(windows, key=lambda d: d["winner_counts"][0])["steps"]
    detail = dict(most_winner_changes=steps(*changes), most_steps_without_winner=steps(*lost), last_steps=steps(max(L - 3, 0), L))
    # the single start on the same seed, for the same windows (its own record: K = 1)
    single = mpc_gpu.run_multistart_episodes(x0, GOAL, "RANDOM", offsets=(0.0,), record=[g], **kw)["record"][g]
    d1 = np.linalg.norm(single["simX"][:, :2] - goal, axis=1)
    out.update(group=int(g), steps=int(L), table_row=many["table"][g].tolist(), single_start_steps=int(single["u"].shape[0]),
               single_start_dist_every_25=[float(v) for v in d1[::25]], steps_without_winner=int((win < 0).sum()), winner_changes=int(change.sum()),
               steps_won_by_member=np.bincount(win + 1, minlength=6).tolist(), first_step_with_margin_below_zero=int(np.argmax(margin <= 0)) if (margin <= 0).any() else None,
               step_of_least_dist=int(np.argmin(dist)), least_dist=float(dist.min()), windows=windows, detail=detail)
    print(json.dumps({k: v for k, v in out.items() if k not in ("windows", "detail")}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["a", "b", "c"], action="append")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--seeds", type=int, default=100)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--this-first", action="store_true")
    ap.add_argument("--out", default=os.path.join(measure.ROOT, "profiles", "multistart_record_rates.json"))
    a = ap.parse_args()
    parts = a.part or (["a", "b"] + (["c"] if a.parent_lib else []))
    res = measure.read_json(a.out)
    if set(parts) & {"a", "b"}:
        torch = measure.require_gpu()
        import mpc_gpu
        for part, name, fn in (("a", "step_times", step_times), ("b", "losing_episode", losing_episode)):
            if part in parts:
                res[name] = fn(a, torch, mpc_gpu)
                measure.write_json(a.out, res)
    if "c" in parts:
        res["bench"] = measure.bench_ab(a.parent_lib, a.bench_rounds, a.this_first)
    measure.write_json(a.out, res)


if __name__ == "__main__":
    main()
