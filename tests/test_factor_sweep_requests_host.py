"""The packed-requests net of the factor sweep without a GPU (factor_sweep_requests_cases.py): from the dynamically inconsistent starts of the
table the oracle ALONE returns status 0 below the iteration cap on every instance of every row on all three solves, so the GPU comparison of
test_gpu_factor_sweep_requests.py has nothing to adjudicate that the oracle's own convergence would explain; and the affine entry that travels with
the relocated row of W~ (b_t[4], the residual of the last state's dynamics) is non-zero in every stage of every start."""
import numpy as np
import pytest

import factor_sweep_live_rows_cases as lc
import factor_sweep_requests_cases as rc
from helpers import oracle_P


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


@pytest.mark.parametrize("row", rc.ROWS, ids=[r["id"] for r in rc.ROWS])
def test_oracle_alone_converges_from_the_inconsistent_starts(orc, row):
    x0, goal, obst = rc.batch(row)
    cfg = orc.config(row["N"], row["no"], row["Tf"])
    res = lc.oracle_three_solves(orc, cfg, row, x0, oracle_P(orc, cfg, obst), goal)
    got = tuple(int((o["status"] == 0).sum()) for _, _, o in res)
    assert got == row["ok"] == (row["B"],) * 3, (row["id"], got)
    assert max(int(o["iters"].max()) for _, _, o in res) < cfg.qp_iter_max
    dt = row["Tf"] / row["N"]
    for X0, U0, _ in res:       # b_t[4] = f(x_t, u_t)[4] - x_{t+1}[4], the word staged beside row 4 of W~_t, in every stage of every instance
        for b in range(row["B"]):
            r4 = [orc.dynamics(X0[b, t], U0[b, t], dt)[0][4] - X0[b, t + 1, 4] for t in range(row["N"])]
            assert np.abs(r4).min() > 0.0, (row["id"], b)


def test_the_table():
    assert [r["N"] for r in rc.ROWS] == [2, 3, 20, 21] and all(r["B"] == 8 and r["no"] == 3 for r in rc.ROWS)
    assert lc.NOISE == 0.2
    seeds = [lc.noise_seed(r, k) for r in rc.ROWS for k in range(3)]
    assert len(set(seeds)) == len(seeds)
