#!/usr/bin/env python3
"""Closed-loop solve rate with 15 to 30 obstacles (the multi-wavefront solve kernel, rti_wide_kernel): N in {10, 20, 30} x n_obst in {15, 20, 30}
at batch 1024 and 16384.  One fused control step (look-ahead, solve, plant, obstacle motion, shift) per launch on the reference's RANDOM draws,
timed with HIP events around K launches after W warm-up launches; then the CPU oracle's rate on the same cells (rti_solve_batch, 16 threads,
host only, after the GPU part).  Writes the JSON record to the path given by --out (default profiles/wide_obstacle_rates.json).
--only N NO B: one GPU cell, no oracle (for a profiler run).
The protocol is this script's own -- W warm-up launches, a stream synchronise, ONE window, no reps -- so of scripts/measure.py it takes the path prelude and
the JSON write only."""
import argparse
import json
import os
import time

import numpy as np

import measure


def gpu_rate(mpc_gpu, N, no, B, K, W):
    import torch
    from mpc_gpu import _lib
    dev = torch.device("cuda:0")
    with mpc_gpu.BatchedMpc(N, no, 0.1 * N, max_batch=B) as m:
        obst = torch.from_numpy(m.generate_scenarios("RANDOM", B)).to(dev)
        x0 = torch.tensor([-7.0, -7.0, np.pi / 4, 0.0, 0.0], dtype=torch.float64, device=dev).repeat(B, 1)
        goal = torch.tensor([7.0, 7.0], dtype=torch.float64, device=dev).repeat(B, 1)
        X = torch.zeros(B, N + 1, 5, dtype=torch.float64, device=dev); U = torch.zeros(B, N, 2, dtype=torch.float64, device=dev)
        u0 = torch.zeros(B, 2, dtype=torch.float64, device=dev); cost = torch.zeros(B, dtype=torch.float64, device=dev)
        status = torch.zeros(B, dtype=torch.int32, device=dev); iters = torch.zeros(B, dtype=torch.int32, device=dev)
        s = torch.cuda.Stream(device=dev)      # a stream of its own: the launches and the events around them on the same (non-null) stream
        torch.cuda.synchronize()
        m.reset_guess_dev(B, x0, X, U, stream=s.cuda_stream)
        fl = _lib.STEP_SHIFT | _lib.STEP_PLANT | _lib.STEP_OBSTACLES | _lib.STEP_RESET_ON_FAIL
        step = lambda: m.closed_loop_step_dev(B, x0, obst, goal, X, U, u0, cost, status, iters, None, flags=fl, stream=s.cuda_stream)
        for _ in range(W):
            step()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        it_sum = 0
        s.synchronize()
        e0.record(s)
        for _ in range(K):
            step()
        e1.record(s)
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        it_sum = int(iters.sum().item())
        return dict(kernel=m.kernel_name(B), ms_per_step=ms / K, solves_per_s=B * K / (ms * 1e-3), mean_iters_last_step=it_sum / B,
                    status4_last_step=int((status == 4).sum().item()))


def oracle_rate(orc, N, no, B):
    import mpc_gpu
    from mpc_gpu import world
    cfg = orc.config(N, no, 0.1 * N)
    obst = np.stack([world.obstacle_states(world.generate_random_moving_obstacles("RANDOM", n_obst=no, rng=np.random.RandomState(s))) for s in range(B)])
    x0 = np.tile([-7.0, -7.0, np.pi / 4, 0, 0], (B, 1)); goal = np.tile([7.0, 7.0], (B, 1))
    P = np.stack([orc.predict_params(cfg, obst[b]) for b in range(B)])
    X = np.zeros((B, N + 1, 5)); U = np.zeros((B, N, 2))
    for b in range(B):
        X[b], U[b] = orc.initial_guess(cfg, x0[b])
    orc.rti_solve_batch(cfg, x0[:64], P[:64], goal[:64], X[:64], U[:64], nthreads=16)
    t = time.perf_counter()
    orc.rti_solve_batch(cfg, x0, P, goal, X, U, nthreads=16)
    dt = time.perf_counter() - t
    return dict(instances=B, s=dt, solves_per_s=B / dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(measure.ROOT, "profiles", "wide_obstacle_rates.json"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--oracle-instances", type=int, default=1024, help="instances per oracle measurement (its rate does not depend on the batch)")
    ap.add_argument("--only", type=int, nargs=3, metavar=("N", "NO", "B"))
    a = ap.parse_args()
    import mpc_gpu
    mpc_gpu.build()
    if a.only:
        N, no, B = a.only
        print(json.dumps(gpu_rate(mpc_gpu, N, no, B, a.steps, a.warmup)))
        return
    cells = [(N, no) for N in (10, 20, 30) for no in (15, 20, 30)]
    rec = dict(what="fused closed-loop control step, one launch per step, RANDOM draws (seeds 0 .. B-1), HIP events; oracle: rti_solve_batch, 16 threads",
               steps=a.steps, warmup=a.warmup, gpu={}, oracle={})
    for N, no in cells:
        for B in (1024, 16384):
            r = gpu_rate(mpc_gpu, N, no, B, a.steps, a.warmup)
            rec["gpu"][f"N{N}_obst{no}_B{B}"] = r
            print("gpu", N, no, B, r, flush=True)
    from oracle import oracle as orc
    orc.build()
    for N, no in cells:
        r = oracle_rate(orc, N, no, a.oracle_instances)
        rec["oracle"][f"N{N}_obst{no}"] = r
        print("oracle", N, no, r, flush=True)
    measure.write_json(a.out, rec)


if __name__ == "__main__":
    main()
