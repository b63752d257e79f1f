"""Every kernel that runs the row-parallel factor sweep, started from DYNAMICALLY INCONSISTENT iterates (factor_sweep_live_rows_cases.py: the rows of
factor_sweep_cases.ROWS, every start with seeded noise on X).  The sweep computes rows 0..4 of T, M~ and P~ only: the gradient of the cost-to-go lives
in column 5 (lane 5) alone, and with an inconsistent start the affine column of W~ and the gradient are O(noise) in every stage, so the feed-forward
that column carries decides the result -- a wrongly deleted column-5 instruction shows here, where the dynamically consistent starts of
test_gpu_factor_sweep_terms.py could hide it.  Three consecutive solves per row (set_warmstart with the start the oracle was given), judged by
helpers.judge_against_oracle as test_gpu_off_default.judge_solves applies it, the kernel named in the table asserted first.  The oracle alone converges
on every instance of every row (test_factor_sweep_live_rows_host.py), so the whole batch is compared; the adjudication cap is the project's
(helpers.allowed_adjudications)."""
import pytest

import factor_sweep_live_rows_cases as lc
import off_default_cases as oc
from feature_loop import mg
from helpers import oracle_P
from test_gpu_off_default import judge_solves

pytestmark = pytest.mark.gpu


def gpu_three_warm_solves(s, ref, x0, obst, P, goal):
    """the three solves of lc.oracle_three_solves on the handle, each from the oracle's (perturbed) start; the first and third take obstacle states
    (look-ahead in the kernel), the second the explicit P.  Returns [(g, X, U)]."""
    B = x0.shape[0]
    outs = []
    for k, (X0, U0, _) in enumerate(ref):
        s.set_warmstart(X0, U0)
        g = s.solve(x0, P if k == 1 else obst, goal)
        X, U = s.get_traj(B)
        outs.append((g, X, U))
    return outs


@pytest.mark.parametrize("rid", [r["id"] for r in lc.ROWS])
def test_three_solves_from_inconsistent_starts_against_the_oracle(mg, rid):
    mpc_gpu, orc = mg
    row = lc.ROW[rid]
    N, no, B, Tf = row["N"], row["no"], row["B"], row["Tf"]
    x0, goal, obst = lc.batch(row)
    cfg = orc.config(N, no, Tf)
    P = oracle_P(orc, cfg, obst)
    ref = lc.oracle_three_solves(orc, cfg, row, x0, P, goal)
    with mpc_gpu.BatchedMpc(N, no, Tf, max_batch=B) as s:
        name = oc.configure(s, row)                                     # the kernel name first
        assert name == row["name"], (rid, name)
        names = [s.kernel_name(B, lookahead=k != 1) for k in range(3)]
        outs = gpu_three_warm_solves(s, ref, x0, obst, P, goal)
    assert names == [row["name"]] * 3, (rid, names)
    judge_solves(orc, cfg, ref, outs, x0, P, goal, row["ok"], False, f"{rid} {name} noise {lc.NOISE}")
