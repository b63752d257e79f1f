"""The reference's experiment sweep in one process: src/simulation/run_multiple_experiments.py (TF x N_OBST) and
run_experiments_qp_solver.py (QP_ITER), each cell being experiments.py's protocol -- scenarios RANDOM and EDGE, seeds 0 .. seeds - 1,
start [-7, -7, pi/4, 0, 0], goal [7, 7], noisy obstacles, init_guess_when_error, at most max_iter control steps -- run as one batch
per cell on the GPU (run_episodes) and written in the reference's file format (write_experiment), so evaluate_experiments.py's loader reads
the output directory.  N = int(TF * 10) as world_specification.py:44; more than 10 obstacles run on the multi-wavefront solve kernel (N <= 31)."""
import numpy as np

from .episodes import run_episodes, run_seed_sweep, write_experiment

START = (-7.0, -7.0, np.pi / 4, 0.0, 0.0)
GOAL = (7.0, 7.0)


def run_grid(TF=(1, 1.5, 2, 2.5, 3), N_OBST=(10, 15, 20, 25, 30), QP_ITER=(50,), scenarios=("RANDOM", "EDGE"), seeds=100, max_iter=400,
             out_dir="experiments", device=0, slots=None, **episode_kw):
    """Runs every cell (TF, N_OBST, QP_ITER, scenario) and writes `<stamp>_experiment_data.csv` + `<stamp>_experiment_spec.json` per cell into
    out_dir.  Returns a list of dict(spec, stamp, table) in the order the cells ran.
    slots: with more seeds than this many, a cell runs as a sweep through `slots` slots that are refilled on the device (run_seed_sweep: the same rows,
    every slot live until the seeds run out); None: one batch of `seeds` episodes per cell."""
    x0 = np.tile(np.asarray(START, dtype=np.float64), (seeds, 1))
    goal = np.tile(np.asarray(GOAL, dtype=np.float64), (seeds, 1))
    cells = []
    for tf in TF:
        N = int(tf * 10)
        for no in N_OBST:
            for qp in QP_ITER:
                for scen in scenarios:
                    if slots is not None and seeds > slots:
                        r = run_seed_sweep(START, GOAL, scen, (0, seeds), slots, N=N, Tf=float(tf), n_obst=no, max_iter=max_iter, random_move=True,
                                           init_guess_when_error=True, device=device, qp_iter_max=qp, **episode_kw)
                    else:
                        r = run_episodes(x0, goal, scen, N=N, Tf=float(tf), max_iter=max_iter, random_move=True, init_guess_when_error=True,
                                         n_obst=no, first_seed=0, device=device, qp_iter_max=qp, **episode_kw)
                    spec = {"slack": True, "random_move": True, "init_guess": True, "scenario": scen, "TF": tf, "N_SOLV": N, "N_OBST": no, "QP_ITER": qp}
                    stamp = f"grid_{scen}_TF{tf:g}_N{no}_QP{qp}"
                    write_experiment(r["table"], spec, out_dir, stamp=stamp)
                    cells.append(dict(spec=spec, stamp=stamp, table=r["table"]))
    return cells
