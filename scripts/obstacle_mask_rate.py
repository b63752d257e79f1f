"""Solves per second with per-instance obstacle masks (mpc_set_obstacle_mask) on the workloads of DESIGN.md section 5.

For each cell the same seeded batch is solved in four modes: "handle" (the plain handle path), "inst" (per-instance parameters that repeat the handle's
values, no mask), "full" (a mask with every bit set: the same problems and iterations as the two before, so full / inst is the cost of the mask code and
full / handle the cost of the whole path) and "half" (every instance keeps a random half of its obstacles: fewer rows, other problems -- the ratio to
"full" is what a batch gains from rows that are absent).  Each rep is reset_guess + `--solves` warm-started RTI solves through the device API, timed on
the solve stream by scripts/measure.py's protocol (HIP event window, the modes alternating rep by rep).  Writes one JSON (default
profiles/obstacle_mask_rates.json).

    python scripts/obstacle_mask_rate.py [--reps 5] [--solves 20] [--out profiles/obstacle_mask_rates.json]
"""
import argparse
import json
import os

import numpy as np

import measure

CELLS = [("C2", 1024, 20, 3), ("C3", 65536, 20, 3), ("C5", 32768, 50, 10), ("wide", 4096, 30, 20)]
MODES = ("handle", "inst", "full", "half")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solves", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(measure.ROOT, "profiles", "obstacle_mask_rates.json"))
    a = ap.parse_args()
    torch = measure.require_gpu()
    import mpc_gpu
    from helpers import random_batch
    dev = torch.device("cuda", 0)
    rows = []
    for name, B, N, no in CELLS:
        Tf = 0.1 * N
        x0, goal, obst = random_batch(B, no, seed=2024 + B + N)
        rng = np.random.default_rng(B + N + no)
        half = np.zeros((B, no), bool)
        for b in range(B):
            half[b, rng.permutation(no)[: (no + 1) // 2]] = True
        res = {}
        with mpc_gpu.BatchedMpc(N, no, Tf, max_batch=B) as s, measure.own_stream(torch) as st:
            cs = st.cuda_stream
            tx, to, tg = (torch.tensor(v, device=dev) for v in (x0, obst, goal))
            X = torch.zeros((B, N + 1, 5), dtype=torch.float64, device=dev); U = torch.zeros((B, N, 2), dtype=torch.float64, device=dev)
            P = torch.zeros((B, N + 1, no, 2), dtype=torch.float64, device=dev)
            u0 = torch.zeros((B, 2), dtype=torch.float64, device=dev); cost = torch.zeros(B, dtype=torch.float64, device=dev)
            status = torch.zeros(B, dtype=torch.int32, device=dev); iters = torch.zeros(B, dtype=torch.int32, device=dev)
            s.predict_dev(B, to, P, stream=cs)
            W = np.tile([s.cfg.W[k] for k in range(6)], (B, 1)); We = np.tile([s.cfg.We[k] for k in range(4)], (B, 1))
            rs = np.full((B, no), float(s.cfg.r_safe))
            names = {}

            def rep(mode):      # (seconds per solve, mean iterations of the last solve)
                def prepare():
                    s.set_instance_params(**(dict(W=W, We=We, r_safe=rs) if mode == "inst" else {}))
                    s.set_obstacle_mask(np.ones((B, no), bool) if mode == "full" else (half if mode == "half" else None))
                    names[mode] = s.kernel_name(B, lookahead=False)
                    s.reset_guess_dev(B, tx, X, U, stream=cs)
                ms = measure.window(torch, st, lambda: s.solve_dev(B, tx, P, tg, X, U, u0, cost, status, iters, stream=cs), a.solves, prepare)
                return ms / 1e3, float(iters.double().mean())

            runs = measure.alternate({m: (lambda m=m: rep(m)) for m in MODES}, a.reps)
            for mode in MODES:
                sec, spread = measure.summary([r[0] for r in runs[mode]])
                res[mode] = dict(kernel=names[mode], solves_per_s=B / sec, spread=spread, mean_iters_last_solve=float(np.mean([r[1] for r in runs[mode]])))
        rate = lambda m: res[m]["solves_per_s"]
        res["full_over_inst"] = rate("full") / rate("inst")
        res["full_over_handle"] = rate("full") / rate("handle")
        res["half_over_full"] = rate("half") / rate("full")
        rows.append(dict(cell=name, batch=B, N=N, n_obst=no, **res))
        print(json.dumps(rows[-1]), flush=True)
    measure.write_json(a.out, dict(reps=a.reps, solves_per_rep=a.solves, cells=rows))


if __name__ == "__main__":
    main()
