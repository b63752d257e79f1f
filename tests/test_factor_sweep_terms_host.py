"""The factor-sweep net without a GPU (factor_sweep_cases.py): the oracle alone returns status 0 for every instance of every row on all three solves,
so the GPU comparison of test_gpu_factor_sweep_terms.py has nothing to adjudicate that the oracle's own convergence would explain."""
import pytest

import factor_sweep_cases as fc
import off_default_cases as oc
from helpers import oracle_P


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


@pytest.mark.parametrize("row", fc.ROWS, ids=[r["id"] for r in fc.ROWS])
def test_oracle_alone_converges_on_every_instance(orc, row):
    x0, goal, obst = fc.batch(row)
    cfg = orc.config(row["N"], row["no"], row["Tf"])
    res = oc.oracle_three_solves(orc, cfg, x0, oracle_P(orc, cfg, obst), goal)
    got = tuple(int((o["status"] == 0).sum()) for _, _, o in res)
    assert got == row["ok"] == (row["B"],) * 3, (row["id"], got)
    assert max(int(o["iters"].max()) for _, _, o in res) < cfg.qp_iter_max      # nobody at the iteration cap: no status borderline to allow


def test_the_table_covers_what_it_says():
    assert sorted({r["N"] for r in fc.ROWS}) == [2, 3, 20, 21, 47]
    assert all(8 <= r["B"] <= 16 for r in fc.ROWS)
    off = [r["id"] for r in fc.ROWS if abs(r["Tf"] / r["N"] - 0.1) > 1e-3]
    assert off == ["split3-n20-dt"] and fc.ROW["split3-n20-dt"]["Tf"] == 0.15 * 20
