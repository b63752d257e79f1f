"""Solves per second of the fused closed loop with per-instance box bounds (mpc_set_instance_bounds) on the workloads of DESIGN.md section 5.

For each cell the same seeded batch runs `--steps` fused control steps (mpc_closed_loop_step_dev: look-ahead, solve, plant, obstacle motion, shift) in two
modes on ONE handle: "mask" (a mask with every bit set and nothing else: the level-3 kernel) and "bounds" (the handle's own bounds tiled through
mpc_set_instance_bounds on top of it: the level-4 kernel, the same problems and iterations) -- bounds / mask is the cost of reading the bounds from the
table.  Each rep restarts from the same state; timed on the step's stream by scripts/measure.py's protocol (HIP event window, rep 0 a warm-up of both
modes, the modes alternating rep by rep).
`--cell` runs one cell (a caller that wants every cell under a time limit of its own starts one process per cell); the JSON (default
profiles/instance_bounds_rates.json) is merged cell by cell.

    python scripts/instance_bounds_rate.py [--cell C2] [--reps 5] [--steps 20] [--out profiles/instance_bounds_rates.json]
"""
import argparse
import json
import os

import numpy as np

import measure

CELLS = [("C2", 1024, 20, 3), ("C3", 65536, 20, 3), ("C5", 32768, 50, 10)]
MODES = ("mask", "bounds")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell", choices=[c[0] for c in CELLS], action="append")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(measure.ROOT, "profiles", "instance_bounds_rates.json"))
    a = ap.parse_args()
    torch = measure.require_gpu()
    import mpc_gpu
    from helpers import random_batch
    L = mpc_gpu._lib
    dev = torch.device("cuda", 0)
    rows = []
    for name, B, N, no in CELLS:
        if a.cell and name not in a.cell:
            continue
        x0, goal, obst = random_batch(B, no, seed=2024 + B + N)
        x0[:, 3:] = 0.0
        res = {}
        with mpc_gpu.BatchedMpc(N, no, 0.1 * N, max_batch=B) as s, measure.own_stream(torch) as st:
            cs = st.cuda_stream
            tx0, to0, tg = (torch.tensor(v, device=dev) for v in (x0, obst, goal))
            tx, to = tx0.clone(), to0.clone()
            X = torch.zeros((B, N + 1, 5), dtype=torch.float64, device=dev); U = torch.zeros((B, N, 2), dtype=torch.float64, device=dev)
            u0 = torch.zeros((B, 2), dtype=torch.float64, device=dev)
            status = torch.zeros(B, dtype=torch.int32, device=dev); iters = torch.zeros(B, dtype=torch.int32, device=dev)
            table = torch.tensor(mpc_gpu.pack_instance_bounds(s.cfg, B), device=dev)
            s.set_obstacle_mask(np.ones((B, no), bool))
            names, last = {}, {}

            def rep(mode):      # (seconds per control step, mean iterations of the last step)
                def prepare():
                    s.set_instance_bounds_dev(table if mode == "bounds" else None)
                    names[mode] = s.kernel_name(B)
                    tx.copy_(tx0); to.copy_(to0)
                    s.reset_guess_dev(B, tx, X, U, stream=cs)
                step = lambda: s.closed_loop_step_dev(B, tx, to, tg, X, U, u0, None, status, iters, flags=L.STEP_SHIFT | L.STEP_PLANT | L.STEP_OBSTACLES, stream=cs)
                ms = measure.window(torch, st, step, a.steps, prepare)
                last[mode] = tx.clone()
                return ms / 1e3, float(iters.double().mean())

            runs = measure.alternate({m: (lambda m=m: rep(m)) for m in MODES}, a.reps)
            for mode in MODES:
                sec, spread = measure.summary([r[0] for r in runs[mode]])
                res[mode] = dict(kernel=names[mode], solves_per_s=B / sec, spread=spread, mean_iters_last_step=float(np.mean([r[1] for r in runs[mode]])))
            res["same_final_state"] = bool(torch.equal(last["mask"], last["bounds"]))      # the two modes ran the same problems
        res["bounds_over_mask"] = res["bounds"]["solves_per_s"] / res["mask"]["solves_per_s"]
        rows.append(dict(cell=name, batch=B, N=N, n_obst=no, **res))
        print(json.dumps(rows[-1]), flush=True)
    measure.merge_cells(a.out, dict(reps=a.reps, steps_per_rep=a.steps), rows, [c[0] for c in CELLS])


if __name__ == "__main__":
    main()
