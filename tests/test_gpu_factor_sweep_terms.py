"""Every kernel that runs the row-parallel factor sweep (rowpar_factor: out-of-place first terms of M~ = H~aug + W~' T with the constants 1 and dt;
rowpar_factor_fast / _fast_c: the same term order as one asm block; rti_wide_kernel: the copied column and term order of earlier builds) against the
oracle, at the horizons where the sweep's control flow differs (factor_sweep_cases.py).  Three consecutive solves per row -- a cold start, then two from the oracle's shifted iterate -- under
helpers.judge_against_oracle as test_gpu_off_default.py uses it, the kernel named in the table asserted first.  The oracle alone converges on every
instance of every row (test_factor_sweep_terms_host.py), so the whole batch is compared and nothing may be adjudicated away from the GPU's own error:
the cap is the project's (helpers.allowed_adjudications: 0.02 % of a batch, never fewer than 2)."""
import pytest

import factor_sweep_cases as fc
import off_default_cases as oc
from feature_loop import mg
from helpers import oracle_P
from test_gpu_off_default import gpu_three_solves, judge_solves

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rid", [r["id"] for r in fc.ROWS])
def test_three_solves_against_the_oracle(mg, rid):
    mpc_gpu, orc = mg
    row = fc.ROW[rid]
    N, no, B, Tf = row["N"], row["no"], row["B"], row["Tf"]
    x0, goal, obst = fc.batch(row)
    cfg = orc.config(N, no, Tf)
    P = oracle_P(orc, cfg, obst)
    ref = oc.oracle_three_solves(orc, cfg, x0, P, goal)
    with mpc_gpu.BatchedMpc(N, no, Tf, max_batch=B) as s:
        name = oc.configure(s, row)                                     # the kernel name first
        assert name == row["name"], (rid, name)
        names = [s.kernel_name(B, lookahead=k != 1) for k in range(3)]  # (the second solve is given the look-ahead: the same kernel there)
        outs = gpu_three_solves(s, ref, x0, obst, P, goal)
    assert names == [row["name"]] * 3, (rid, names)
    judge_solves(orc, cfg, ref, outs, x0, P, goal, row["ok"], False, f"{rid} {name}")
