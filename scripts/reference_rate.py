"""Solves per second with and without a per-stage reference (mpc_set_reference) on the workloads of DESIGN.md section 5.

For each cell the same seeded batch is solved with the goal path and with a reference path (a smooth random path per instance, one row per
stage, device resident); each rep is reset_guess + `--solves` warm-started RTI solves through the device API, timed on the solve stream by
scripts/measure.py's protocol (HIP event window, the two modes alternating rep by rep).  Writes one JSON (default profiles/reference_rates.json).

    python scripts/reference_rate.py [--reps 5] [--solves 20] [--out profiles/reference_rates.json]
"""
import argparse
import json
import os

import numpy as np

import measure

CELLS = [("C2", 1024, 20, 3), ("C3", 65536, 20, 3), ("C5", 32768, 50, 10), ("wide", 4096, 30, 20)]
MODES = ("goal", "ref")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solves", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(measure.ROOT, "profiles", "reference_rates.json"))
    a = ap.parse_args()
    torch = measure.require_gpu()
    import mpc_gpu
    from helpers import random_batch
    dev = torch.device("cuda", 0)
    rows = []
    for name, B, N, no in CELLS:
        Tf = 0.1 * N
        x0, goal, obst = random_batch(B, no, seed=2024 + B + N)
        rng = np.random.default_rng(B + N)
        t = np.linspace(0, 1, N + 1)
        yref = np.zeros((B, N + 1, 6))
        yref[:, :, 0] = goal[:, :1] + rng.uniform(-1, 1, (B, 1)) * np.sin(t)
        yref[:, :, 1] = goal[:, 1:] + rng.uniform(-1, 1, (B, 1)) * np.cos(t)
        yref[:, :, 2] = rng.uniform(-0.5, 0.5, (B, 1))
        res = {}
        with mpc_gpu.BatchedMpc(N, no, Tf, max_batch=B) as s, measure.own_stream(torch) as st:
            cs = st.cuda_stream
            tx, to, tg = (torch.tensor(v, device=dev) for v in (x0, obst, goal))
            ty = torch.tensor(yref, device=dev)
            X = torch.zeros((B, N + 1, 5), dtype=torch.float64, device=dev); U = torch.zeros((B, N, 2), dtype=torch.float64, device=dev)
            P = torch.zeros((B, N + 1, no, 2), dtype=torch.float64, device=dev)
            u0 = torch.zeros((B, 2), dtype=torch.float64, device=dev); cost = torch.zeros(B, dtype=torch.float64, device=dev)
            status = torch.zeros(B, dtype=torch.int32, device=dev); iters = torch.zeros(B, dtype=torch.int32, device=dev)
            s.predict_dev(B, to, P, stream=cs)
            names = {}

            def rep(mode):      # (seconds per solve, mean iterations of the last solve)
                def prepare():
                    s.set_reference(ty if mode == "ref" else None)
                    names[mode] = s.kernel_name(B, lookahead=False)
                    s.reset_guess_dev(B, tx, X, U, stream=cs)
                ms = measure.window(torch, st, lambda: s.solve_dev(B, tx, P, tg, X, U, u0, cost, status, iters, stream=cs), a.solves, prepare)
                return ms / 1e3, float(iters.double().mean())

            runs = measure.alternate({m: (lambda m=m: rep(m)) for m in MODES}, a.reps)
            for mode in MODES:
                sec, spread = measure.summary([r[0] for r in runs[mode]])
                res[mode] = dict(kernel=names[mode], solves_per_s=B / sec, spread=spread, mean_iters_last_solve=float(np.mean([r[1] for r in runs[mode]])))
        res["ref_over_goal"] = res["ref"]["solves_per_s"] / res["goal"]["solves_per_s"]
        rows.append(dict(cell=name, batch=B, N=N, n_obst=no, **res))
        print(json.dumps(rows[-1]), flush=True)
    measure.write_json(a.out, dict(reps=a.reps, solves_per_rep=a.solves, cells=rows))


if __name__ == "__main__":
    main()
