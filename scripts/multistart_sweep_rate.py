"""What the refill for multi-start groups buys at the reference's 1000 seeds (mpc_group_refill_dev, run_multistart_sweep; DESIGN.md sections 4n and 5k).
The method is section 5j's: wall time around a driver call that ends in a synchronise, or HIP events on the driver's stream; one warm-up rep; median and
spread (max - min over median) of `--reps` reps.  Handles are made in front of the timed region (solver=), so a call's time is its control steps.

(a) 1000 seeds (start [-7, -7, pi/4, 0, 0], goal [7, 7], RANDOM, 5 obstacles, K = 5, the cost rule, incumbent_margin 0 and 0.5, 400 steps at most) through
    run_multistart_episodes on ONE batch of 1000 groups, against run_multistart_sweep through 125, 250 and 500 group slots: wall time, control steps
    launched, member slots launched (control steps x groups x K) and member solves (K x the episodes' control steps).
(b) the columns of section 5j(b) from each sweep, next to the batch's; rows whose flags or step counts differ from the batch's are COUNTED and recorded,
    with the largest difference over the rows that agree -- not asserted (three member solves share a wavefront: an episode's rounding depends on its
    neighbours, and a closed loop of hundreds of steps may amplify it).
(c) the refill's share of a control step in steady state, 250 groups of K = 5 (HIP events, `--launches` consecutive calls): the refill with nothing finished
    (what all but a few control steps of a sweep launch), the refill that starts a seed in every group (the first call of a sweep), and the control step
    behind it (noise draw + member solve + group tail).
(d) bench.py --gpus 1 --steps 20 --warmup 5 with the parent commit's library (`--parent-lib PATH`) and this one's, alternating, parent first
    (scripts/measure.py's bench_ab): the flagship path launches nothing of this change.

    python scripts/multistart_sweep_rate.py [--part a] [--part c] [--part d --parent-lib PATH] [--out profiles/multistart_sweep_rates.json]
(parts a and b are one run.)"""
import argparse
import json
import os

import numpy as np

import measure

SLOTS = (125, 250, 500)
MARGINS = (0.0, 0.5)
MAX_ITER = 400


def columns(r):
    """section 5j(b)'s columns of one run's result"""
    tb = r["table"]
    reached, hit = tb[:, 1] == 1, tb[:, 0] == 1
    return dict(reached=int(reached.sum()), hit=int(hit.sum()), reached_without_hit=int((reached & ~hit).sum()), out_of_bounds=int(tb[:, 5].sum()),
                mean_steps_of_reached=float(tb[reached, 4].mean()) if reached.any() else None, min_margin_median=float(np.median(tb[:, 2])),
                steps_without_winner=int(r["lost_steps"].sum()), steps_won_by_another_member=int(r["switched_steps"].sum()))


def timed(reps, call):
    """reps + 1 calls, the first a warm-up: (the last result, median wall seconds, spread); the call ends in a synchronise of its own"""
    runs = measure.alternate(dict(call=lambda: measure.wall(call)), reps)["call"]
    return (runs[-1][1],) + measure.summary([seconds for seconds, _ in runs])


def sweep_against_batch(a, torch, mpc_gpu):
    from mpc_gpu.experiments import GOAL, START
    from mpc_gpu import world as w
    offsets = mpc_gpu.multistart.DEFAULT_OFFSETS
    K, G = len(offsets), a.seeds
    prob = dict(offsets=offsets, select_by="cost", max_iter=MAX_ITER)
    out = []
    for m_inc in MARGINS:
        with mpc_gpu.MultiStartMpc(w.N_SOLV, w.N_OBST, w.TF, scenarios=G, offsets=offsets, incumbent_margin=m_inc) as ms:
            ref, wall, spread = timed(a.reps, lambda: mpc_gpu.run_multistart_episodes(np.tile(START, (G, 1)), GOAL, "RANDOM", incumbent_margin=m_inc, first_seed=0,
                                                                                      solver=ms, **prob))
        lengths = ref["table"][:, 4] + ref["table"][:, 1]
        row = dict(incumbent_margin=m_inc, K=K, seeds=G, max_iter=MAX_ITER, N=w.N_SOLV, n_obst=w.N_OBST, reps=a.reps,
                   batch=dict(groups=G, wall_s=wall, wall_spread=spread, control_steps=ref["steps_run"], member_slots_launched=ref["steps_run"] * G * K,
                              member_solves=ref["solves"], useful_share=ref["solves"] / (ref["steps_run"] * G * K), mean_episode_steps=float(lengths.mean()),
                              longest_episode_steps=int(lengths.max()), **columns(ref)), sweeps=[])
        print(json.dumps(dict(row, sweeps=None)), flush=True)
        for S in SLOTS:
            with mpc_gpu.MultiStartMpc(w.N_SOLV, w.N_OBST, w.TF, scenarios=S, offsets=offsets, incumbent_margin=m_inc) as ms:
                r, wall, spread = timed(a.reps, lambda: mpc_gpu.run_multistart_sweep(START, GOAL, "RANDOM", (0, G), S, incumbent_margin=m_inc, solver=ms, **prob))
            same = (r["table"][:, [0, 1, 4, 5]] == ref["table"][:, [0, 1, 4, 5]]).all(axis=1)
            d = np.abs(np.where(r["table"][same] == ref["table"][same], 0.0, r["table"][same] - ref["table"][same]))
            row["sweeps"].append(dict(group_slots=S, wall_s=wall, wall_spread=spread, wall_over_batch=wall / row["batch"]["wall_s"], control_steps=r["steps_run"],
                                      member_slots_launched=r["steps_run"] * S * K, member_solves=r["solves"], useful_share=r["solves"] / (r["steps_run"] * S * K),
                                      member_slots_over_batch=r["steps_run"] * S / (ref["steps_run"] * G), rows_differing_from_the_batch=int((~same).sum()),
                                      largest_difference_over_agreeing_rows=float(d.max()) if d.size else None, **columns(r)))
            print(json.dumps(row["sweeps"][-1]), flush=True)
        out.append(row)
    return dict(runs=out)


def refill_share(a, torch, mpc_gpu):
    from mpc_gpu.experiments import GOAL, START
    from mpc_gpu import world as w
    from mpc_gpu.multistart import _sweep_state, sweep_arguments
    S, L = 250, a.launches
    with mpc_gpu.MultiStartMpc(w.N_SOLV, w.N_OBST, w.TF, scenarios=S) as ms:
        args = sweep_arguments(START, GOAL, "RANDOM", (0, S * (a.reps + 1)), S, offsets=ms.offsets_host, max_iter=MAX_ITER, solver=ms)
        with measure.own_stream(torch, ms.stream) as stream:
            cs = stream.cuda_stream

            def us(body, n, prepare=None):      # microseconds per call
                return lambda: 1e3 * measure.window(torch, stream, body, n, prepare)

            def step():
                ms.inner.noise_draw_dev(S, st.state, st.nbuf, ep_flags=ms.ep_flags, stream=cs)
                ms.step_fused(st.x, st.obst, st.goal, noise=st.nbuf)

            ms.restart()
            st = _sweep_state(torch, ms, args, "RANDOM")
            refill = lambda: st.refill(cs)
            # in front of the first window every group has ended: the refill parks it and starts a seed in it
            t = measure.alternate(dict(refill_starting_every_group=us(refill, 1, lambda: ms.ep_flags.fill_(1)), refill_nothing_finished=us(refill, L),
                                       control_step=us(step, L)), a.reps)
            assert int(st.cursor[0].item()) == S * (a.reps + 1) and not bool((ms.ep_flags & 1).any())      # every timed refill did what its name says
    med, spread = measure.summaries(t)
    return dict(group_slots=S, K=ms.K, reps=a.reps, calls_per_rep=L, us=med, spread=spread,
                share_of_a_control_step=med["refill_nothing_finished"] / (med["refill_nothing_finished"] + med["control_step"]),
                share_when_every_group_starts=med["refill_starting_every_group"] / (med["refill_starting_every_group"] + med["control_step"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["a", "c", "d"], action="append")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--seeds", type=int, default=1000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--this-first", action="store_true")
    ap.add_argument("--out", default=os.path.join(measure.ROOT, "profiles", "multistart_sweep_rates.json"))
    a = ap.parse_args()
    parts = a.part or (["a", "c"] + (["d"] if a.parent_lib else []))
    res = measure.read_json(a.out)
    if set(parts) & {"a", "c"}:
        torch = measure.require_gpu()
        import mpc_gpu
        for part, name, fn in (("a", "sweep_against_batch", sweep_against_batch), ("c", "refill_share", refill_share)):
            if part in parts:
                res[name] = fn(a, torch, mpc_gpu)
    if "d" in parts:
        res["bench"] = measure.bench_ab(a.parent_lib, a.bench_rounds, a.this_first)
    measure.write_json(a.out, res)


if __name__ == "__main__":
    main()
