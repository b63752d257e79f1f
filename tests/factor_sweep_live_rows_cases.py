"""Case table of the live-rows net of the factor sweep (test_factor_sweep_live_rows_host.py, test_gpu_factor_sweep_live_rows.py).  The sweep keeps the
gradient of the cost-to-go once -- as column 5 of P~ (lane 5, registers 0..4) -- and no longer as row 5 (register 5 of every lane): rows 0..4 of T,
M~ and P~ are all it computes (rowpar_factor, rti_kernel.hpp).  What the deleted row duplicated is the feed-forward, so the rows of
factor_sweep_cases.ROWS (imported, not copied) are started from a DYNAMICALLY INCONSISTENT iterate: the initial guess (first solve) or the oracle's
shifted iterate (second, third) plus seeded noise on X.  Then the affine column b_t of W~ and the gradient are O(noise) in every stage and the
feed-forward carries the result; factor_sweep_cases starts dynamically consistent (b_t = 0 on a cold start), where a wrongly deleted column-5
instruction could hide.

NOISE: amplitude of the uniform noise on every state of every stage but x_0 (which the solve pins to the measured state anyway).  Chosen by the rule
"start at 0.2 and halve until the oracle ALONE returns status 0 below the iteration cap on every instance of every row, on all three solves";
the host test asserts that for the value recorded here.  Seeds: 1000 + 10 * (the row's seed) + the solve's index."""
import numpy as np

import factor_sweep_cases as fc

ROWS = fc.ROWS
ROW = fc.ROW
NOISE = 0.2


def batch(row):
    return fc.batch(row)


def noise_seed(row, k):
    return 1000 + 10 * row["seed"] + k


def perturbed(row, k, X):
    """X (B, N + 1, 5) plus the seeded noise of solve k; x_0 stays"""
    rng = np.random.default_rng(noise_seed(row, k))
    Xn = np.array(X, dtype=np.float64, copy=True)
    Xn[:, 1:, :] += rng.uniform(-NOISE, NOISE, Xn[:, 1:, :].shape)
    return Xn


def oracle_three_solves(orc, cfg, row, x0, P, goal):
    """the oracle alone: from the initial guess, then twice from its own shifted iterate, each start with perturbed() states.
    Returns [(X0, U0, result)] per solve, X0 the perturbed start the GPU is given too."""
    B = x0.shape[0]
    X, U = zip(*[orc.initial_guess(cfg, x) for x in x0])
    X, U = np.stack(X), np.stack(U)
    out = []
    for k in range(3):
        X = perturbed(row, k, X)
        o = orc.rti_solve_batch(cfg, x0, P, goal, X, U)
        out.append((X, U, o))
        X, U = o["X"].copy(), o["U"].copy()
        for b in range(B):
            X[b], U[b] = orc.shift(cfg, X[b], U[b])
    return out
