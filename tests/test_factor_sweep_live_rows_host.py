"""The live-rows net of the factor sweep without a GPU (factor_sweep_live_rows_cases.py): with the dynamically inconsistent starts of the table the
oracle ALONE returns status 0 below the iteration cap for every instance of every row on all three solves, so the GPU comparison of
test_gpu_factor_sweep_live_rows.py has nothing to adjudicate that the oracle's own convergence would explain -- and the starts are what they claim
to be: the dynamics residual of every start is of the order of the noise, not zero."""
import numpy as np
import pytest

import factor_sweep_cases as fc
import factor_sweep_live_rows_cases as lc
from helpers import oracle_P


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


@pytest.mark.parametrize("row", lc.ROWS, ids=[r["id"] for r in lc.ROWS])
def test_oracle_alone_converges_from_the_inconsistent_starts(orc, row):
    x0, goal, obst = lc.batch(row)
    cfg = orc.config(row["N"], row["no"], row["Tf"])
    res = lc.oracle_three_solves(orc, cfg, row, x0, oracle_P(orc, cfg, obst), goal)
    got = tuple(int((o["status"] == 0).sum()) for _, _, o in res)
    assert got == row["ok"] == (row["B"],) * 3, (row["id"], got)
    assert max(int(o["iters"].max()) for _, _, o in res) < cfg.qp_iter_max      # nobody at the iteration cap: no status borderline to allow


@pytest.mark.parametrize("row", lc.ROWS, ids=[r["id"] for r in lc.ROWS])
def test_the_starts_are_dynamically_inconsistent(orc, row):
    """the initial guess is dynamically consistent (b_t = 0 in every stage); the starts of the table move every state of every stage behind x_0 by
    O(NOISE), independently, so no stage keeps a zero residual"""
    x0, goal, obst = lc.batch(row)
    cfg = orc.config(row["N"], row["no"], row["Tf"])
    X, _ = zip(*[orc.initial_guess(cfg, x) for x in x0])
    X = np.stack(X)
    for k in range(3):
        Xn = lc.perturbed(row, k, X)
        assert np.array_equal(Xn[:, 0], X[:, 0])                       # x_0 stays
        d = np.abs(Xn[:, 1:] - X[:, 1:])
        assert d.max() <= lc.NOISE and np.median(d) > 0.25 * lc.NOISE and d.max(axis=(0, 2)).min() > 0.5 * lc.NOISE      # every stage
        assert not np.array_equal(lc.perturbed(row, (k + 1) % 3, X), Xn)                                            # a seed per solve


def test_the_table_is_the_factor_sweep_table():
    assert lc.ROWS is fc.ROWS and lc.ROW is fc.ROW
    assert 0.0 < lc.NOISE <= 0.2 and np.log2(0.2 / lc.NOISE) == round(np.log2(0.2 / lc.NOISE))       # 0.2, halved some number of times
    seeds = [lc.noise_seed(r, k) for r in lc.ROWS for k in range(3)]
    assert len(set(seeds)) == len(seeds)
