"""What the guess family from geometry costs and what it buys (mpc_set_guess_geometry, mpc_seed_guesses_geom_dev, MultiStartMpc(guess_geometry=...);
DESIGN.md sections 4o and 5l).

(a) LAUNCH TIMES, the protocol of multistart_rate.py (a): `--launches` back-to-back launches between two HIP events on the object's stream, `--reps` times
    after one warm-up rep, median and spread (max - min over median).  For G groups of K = 5 members (G K = 5120 and 65535; N = 20; 3 and 10 obstacles;
    random scenarios of tests/helpers.random_batch) the three launches that seed members:
      seed    the stand-alone seed launch (mpc_seed_guesses_dev; with the mode on mpc_seed_guesses_geom_dev);
      step    mpc_group_step_dev on the costs of one member solve, the plant coasting (u0 = 0) so that no group finishes while it is timed;
      refill  mpc_group_refill_dev with every group finished (a fill of the flag words in front of each call, timed with it): every group starts a seed.
    Each with the mode off and, where the library has it, on.  `--label parent` with MPC_GPU_LIB naming the parent commit's library records the parent's
    three launches (there is no mode to switch); the cells of `this` are then compared with them: mode off against the parent is the cost of carrying the
    feature, mode on against the parent the cost of the rule.
(b) CLOSED-LOOP OUTCOME, recorded and not asserted: multistart_rate.py (b)'s protocol (100 seeds, RANDOM, 5 obstacles, N = 20, at most 400 control steps,
    MultiStartMpc.step) with the fixed family against guess_geometry=True at incumbent_margin 0, 0.1 and 0.5, and one row with lead = 0.5; its columns and
    the share of group steps won by a member other than 0, and by a GEOMETRIC member (one whose amplitude the rule set: it differs from its base offset).

    python scripts/multistart_geometry_rate.py [--part a] [--part b] [--label this|parent] [--out profiles/multistart_geometry_rates.json]
"""
import argparse
import json
import os

import numpy as np

import measure

GROUPS = (1024, 13107)      # x K = 5: 5120 and 65535 instances
OBSTACLES = (3, 10)
N, TF = 20, 2.0


def launch_times(a, torch, mpc_gpu):
    from helpers import random_batch
    from mpc_gpu import multistart as msm
    L = mpc_gpu._lib
    has_mode = hasattr(L.lib(), "mpc_set_guess_geometry") and a.label != "parent"
    rows = []
    for no in OBSTACLES:
        for G in GROUPS:
            for mode in ((None, True) if has_mode else (None,)):
                x0, goal, obst = random_batch(G, no, seed=4242 + G)
                x0[:, 3:] = 0.0
                kw = dict(guess_geometry=mode) if has_mode else {}
                with mpc_gpu.MultiStartMpc(N, no, TF, scenarios=G, **kw) as ms:
                    K = ms.K
                    with measure.own_stream(torch, ms.stream) as st:
                        cs = st.cuda_stream
                        dev = ms.dev
                        x, ob, gl = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (x0, obst, goal))
                        ms.step_fused(x, ob, gl)                  # loads and seeds the members, one solve, one group step: every array of the step exists
                        ms.cand_u0.zero_()
                        sa = msm.sweep_arguments(x0[0], goal[0], "RANDOM", (0, G * a.launches), G, max_iter=400)
                        sw = msm._sweep_state(torch, ms, sa, "RANDOM")
                        ms.member_flags.zero_(); ms.ep_flags.zero_()

                        def seed():
                            ms._seed(x, gl, False, cs, ob) if has_mode else ms._seed(x, gl, False, cs)

                        def step():
                            L.check(L.lib().mpc_group_step_dev(ms.inner._h, G, K, ms.cand_cost.data_ptr(), ms.cand_status.data_ptr(), ms.cand_u0.data_ptr(), 0.0, 0,
                                                               x.data_ptr(), ob.data_ptr(), gl.data_ptr(), ms.offsets.data_ptr(), None, 0.1, 2.0, ms.X.data_ptr(),
                                                               ms.U.data_ptr(), ms._out, cs))

                        def refill():
                            ms.ep_flags.fill_(1)
                            sw.refill(cs)

                        def us(body, prepare=None):      # microseconds per launch
                            return lambda: 1e3 * measure.window(torch, st, body, a.launches, prepare)

                        def sweep_reset():
                            sw.cursor.zero_(); sw.slot_seed.fill_(-1); ms.ep_flags.fill_(1)

                        t = measure.alternate(dict(seed=us(seed), step=us(step, lambda: ms.ep_flags.zero_()), refill=us(refill, sweep_reset)), a.reps)
                        started = int(sw.cursor[0].item())
                        torch.cuda.synchronize()
                med, spread = measure.summaries(t)
                cell = dict(label=a.label, mode="on" if mode else "off", groups=G, K=K, instances=G * K, N=N, n_obst=no, us=med, spread=spread,
                            seeds_started_in_the_last_rep=started)
                rows.append(cell)
                print(json.dumps(cell), flush=True)
    return dict(reps=a.reps, launches_per_rep=a.launches, cells=rows)


def closed_loop(a, torch, mpc_gpu):
    from mpc_gpu.experiments import GOAL, START
    from mpc_gpu import world as w
    seeds, max_iter, no = 100, 400, w.N_OBST
    r_hit = w.R_OBST + w.R_ROBOT
    out = []
    five = mpc_gpu.multistart.DEFAULT_OFFSETS
    cases = [(None, m) for m in (0.0, 0.1, 0.5)] + [(True, m) for m in (0.0, 0.1, 0.5)] + [(dict(lead=0.5), 0.0)]
    for geometry, m_inc in cases:
        with mpc_gpu.MultiStartMpc(w.N_SOLV, no, w.TF, scenarios=seeds, offsets=five, incumbent_margin=m_inc, guess_geometry=geometry) as ms:
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
                steps, lost, switched, geometric, run = (torch.zeros(seeds, dtype=torch.int32, device=dev) for _ in range(5))
                margin = torch.full((seeds,), float("inf"), dtype=torch.float64, device=dev)
                held = None                                       # the amplitudes of the members the NEXT solve starts from
                for k in range(max_iter):
                    m.noise_draw_dev(seeds, state, noise, stream=cs)
                    res = ms.step(x, obst, goal, noise=noise, randomness=w.RANDOMNESS, vmax=w.V_MAX_OBST)
                    live = ~reached
                    win = res["winner"].long()
                    if ms.member_offsets is not None and held is not None:
                        amp = held.gather(1, win.clamp(min=0)[:, None])[:, 0]
                        geometric += (live & (win > 0) & (amp != ms.offsets[win.clamp(min=0)])).int()
                    if ms.member_offsets is not None:
                        held = ms.member_offsets.clone()
                    d = torch.linalg.norm(x[:, None, :2] - obst[:, :, :2], dim=2).min(dim=1).values - r_hit
                    margin = torch.where(live, torch.minimum(margin, d), margin)
                    lost += (live & (win < 0)).int(); switched += (live & (win > 0)).int(); run += live.int()
                    now = torch.linalg.norm(x[:, :2] - goal, dim=1) <= w.TOL
                    steps += (live & ~now).int()
                    reached |= now
                    if k % 25 == 24 and bool(reached.all()):
                        break
                torch.cuda.synchronize()
            c = lambda t: t.cpu().numpy()
            reached, steps, margin, total = c(reached), c(steps), c(margin), int(c(run).sum())
            out.append(dict(K=len(five), guess_geometry=ms.guess_geometry, incumbent_margin=m_inc, seeds=seeds, max_iter=max_iter, N=w.N_SOLV, n_obst=no,
                            reached=int(reached.sum()), hit=int((margin <= 0).sum()), reached_without_hit=int((reached & (margin > 0)).sum()),
                            mean_steps_of_reached=float(steps[reached].mean()) if reached.any() else None, min_margin_median=float(np.median(margin)),
                            steps_without_winner=int(c(lost).sum()), group_steps=total, share_won_by_a_member_other_than_0=float(c(switched).sum() / total),
                            share_won_by_a_geometric_member=float(c(geometric).sum() / total) if ms.guess_geometry else None))
            print(json.dumps(out[-1]), flush=True)
    return dict(runs=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["a", "b"], action="append")
    ap.add_argument("--label", choices=["this", "parent"], default="this")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(measure.ROOT, "profiles", "multistart_geometry_rates.json"))
    a = ap.parse_args()
    torch = measure.require_gpu()
    import mpc_gpu
    parts = a.part or ["a", "b"]
    res = measure.read_json(a.out)
    if "a" in parts:
        res.setdefault("launch_times", {})[a.label] = launch_times(a, torch, mpc_gpu)
    if "b" in parts:
        res["closed_loop"] = closed_loop(a, torch, mpc_gpu)
    measure.write_json(a.out, res)


if __name__ == "__main__":
    main()
