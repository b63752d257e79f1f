"""The conditions the SQP loop's GPU tests (test_gpu_sqp.py) rely on, held on the oracle alone: K successive single RTI solves per instance, stopped by
the rule of include/mpc_gpu.h mpc_set_sqp (sqp_cases.oracle_sequence).  No GPU here.

  1. every finite instance has status 0 on every iteration run (the instance with a NaN in x0 has status 4 at once);
  2. no step norm of an iteration run lies in [step_tol / 2, 2 step_tol]: GPU and oracle agree to ~1e-6 per iterate, so the stop decision of no
     instance is a coin flip between them;
  3. three or more different stop counts occur in every case, one instance or more runs all K iterations and one or more stops before K;
  4. on every iteration run the oracle's step is within 1e-7 of the exact solution of the QP it solved (helpers.exact_qp on orc.export_qp), so no
     comparison of a GPU result with this reference needs an adjudication.
These are conditions on the chosen instances and tolerances (sqp_cases.CASES), not measurements; the counts are printed."""
import numpy as np
import pytest

import sqp_cases as sc
from helpers import exact_qp, step_vector


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


def test_the_cases_cover_every_family_and_lane_mapping_of_level_five():
    names = [c["name"] for c in sc.CASES]
    assert len(set(names)) == len(names) == len(sc.CASES)
    assert all(n.endswith(", true" * 5 + ">") for n in names)
    for c in sc.CASES:      # the horizons at which the plan takes the family: three lanes per stage up to 20, two up to 31, one beyond; wide up to 31
        lo, hi = {("split", 3): (2, 20), ("split", 2): (21, 31), ("one", 1): (32, 62), ("wide", 2): (2, 31)}[c["family"], c["lps"]]
        assert lo <= c["N"] <= hi and c["no"] == c["cap"]
    # what the issue lists, and the five-obstacle rows beside it
    assert {(c["family"], c["lps"], c["cap"]) for c in sc.CASES} >= {("split", 3, 3), ("split", 3, 10), ("split", 2, 3), ("split", 2, 10), ("one", 1, 3),
                                                                    ("one", 1, 10), ("wide", 2, 20), ("wide", 2, 32), ("split", 3, 5), ("split", 2, 5)}


@pytest.mark.parametrize("cid", sc.IDS)
def test_statuses_stop_counts_and_the_band_around_the_tolerance(orc, cid):
    c = sc.case(cid)
    r = sc.oracle_sequence(orc, c)
    fin = sc.finite_instances()
    tol = c["step_tol"]
    ran = r["statuses"] >= 0
    assert (r["statuses"][fin][ran[fin]] == 0).all(), r["statuses"]
    assert r["statuses"][sc.NAN_INSTANCE].tolist() == [4] + [-1] * (sc.K - 1) and r["sqp_iters"][sc.NAN_INSTANCE] == 1
    assert np.array_equal(ran.sum(axis=1), r["sqp_iters"])
    norms = r["norms"][fin]
    assert np.isfinite(norms[ran[fin]]).all()
    in_band = (norms >= tol / 2) & (norms <= 2 * tol)      # (NaN -- not run -- compares false)
    counts = r["sqp_iters"][fin]
    nearest = np.nanmin(np.abs(np.log(norms / tol)))
    print(f"SQP-HOST {cid}: step_tol {tol}, stop counts {counts.tolist()}, nearest norm a factor {np.exp(nearest):.2f} from step_tol, "
          f"interior-point iterations {r['iters'][fin].tolist()}")
    assert not in_band.any(), norms[in_band.any(axis=1)]
    assert len(set(counts.tolist())) >= 3 and (counts == sc.K).any() and (counts < sc.K).any(), counts
    # the stop rule itself: an instance that stopped before K did so on a norm at or below the tolerance, and on no earlier one
    for b, k in zip(fin, counts):
        assert (r["norms"][b, :k - 1] > tol).all() and (k == sc.K or r["norms"][b, k - 1] <= tol)


@pytest.mark.parametrize("cid", sc.IDS)
def test_every_oracle_iteration_solves_its_qp_exactly(orc, cid):
    c = sc.case(cid)
    inp = sc.inputs(orc, c)
    r = sc.oracle_sequence(orc, c)
    worst, n = 0.0, 0
    for b in sc.finite_instances():
        its = r["iterates"][b] + [(r["X"][b], r["U"][b])]
        for (Xa, Ua), (Xb, Ub) in zip(its[:-1], its[1:]):
            q = orc.export_qp(inp["cfg"], inp["x0"][b], inp["P"][b], inp["goal"][b], Xa, Ua)
            vo = step_vector(inp["N"], Xa, Ua, Xb, Ub)
            vex, ok, info = exact_qp(q, vo)
            assert ok, (b, info)
            d = float(np.abs(vo - vex).max())
            worst, n = max(worst, d), n + 1
            assert d <= 1e-7, (b, d, info)
    print(f"SQP-HOST {cid}: {n} oracle iterations against the exact QP solution, worst distance {worst:.2e}")
