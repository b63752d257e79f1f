"""The feature-level kernel sweep without a GPU (feature_kernel_cases.py): the enumeration is the written-out list of 78 names, every name's level is
its case's, and the oracle alone converges on every non-idle instance of every case on both solves -- a condition of the GPU test's judgement, not
a measurement.  The counts it prints are the ones of DESIGN.md section 4g."""
import numpy as np
import pytest

import feature_kernel_cases as fk
from feature_loop import level_of


@pytest.fixture(scope="module")
def orc(built):
    from oracle import oracle
    return oracle


def test_enumeration_is_the_written_out_list():
    cases = fk.enumerate_cases()
    names = [c["name"] for c in cases]
    assert len(names) == 78 and len(set(names)) == 78
    assert names == fk.NAMES
    per_level = {lv: sum(c["level"] == lv for c in cases) for lv in fk.LEVELS}
    assert per_level == {1: 28, 2: 28, 3: 11, 4: 11}
    for lv, fam, n in ((1, "one", 6), (1, "split", 18), (1, "wide", 4), (3, "one", 3), (4, "split", 6), (4, "wide", 2)):
        assert len(fk.cases_of(fam, lv)) == n
    # the 22 (N, n_obst) pairs: every capacity, full and partly empty, at every horizon class
    pairs = {(c["N"], c["no"]) for c in cases}
    assert pairs == {(N, no) for N in (20, 30, 50) for no in (3, 5, 10, 2, 4, 7)} | {(20, 20), (20, 15), (31, 32), (31, 27)}


def test_every_name_has_its_case_level():
    for c in fk.enumerate_cases():
        assert level_of(c["name"]) == c["level"], c
        assert c["name"].startswith({"one": "rti_solve_kernel<", "split": "rti_split_kernel<", "wide": "rti_wide_kernel<"}[c["family"]])
        # below level 3 the run-time row count is the partly empty handle; from level 3 on every handle
        assert (c["no"] < c["cap"]) == (c["masked"] if c["level"] <= 2 else c["level"] == 3), c


def test_inputs_have_the_shape_the_sweep_relies_on(orc):
    for c in (fk.cases_of("split", 4)[0], fk.cases_of("wide", 3)[0], fk.cases_of("one", 1)[1]):
        inp = fk.inputs(orc, c)
        N, no = c["N"], c["no"]
        assert sorted(np.bincount(inp["group"]).tolist()) == [3, 3, 3, 3]
        assert np.linalg.norm(inp["x0"][0, :2] - inp["goal"][0]) < 0.08 and inp["ep_flags"].tolist() == [0, 1] + [0] * 10
        own = inp["group"] != 0
        assert (inp["offset"][~own] == 0).all() and len(set(inp["offset"][own].tolist())) >= 2 and inp["offset"].max() <= 3
        for b in range(fk.B):      # the goal row at and behind the offset, the decoy in front of it
            o = inp["offset"][b]
            assert np.array_equal(inp["yref"][b, o:, :2], np.tile(inp["goal"][b], (inp["T"] - o, 1))) and (inp["yref"][b, :, 2:] == 0).all()
            assert np.array_equal(inp["yref"][b, :o, :2], np.tile(inp["goal"][b] + (5.0, -5.0), (o, 1)))
        g0 = inp["groups"][0]
        base = orc.config(N, no, 0.1 * N)
        assert g0["mask"].all() and (g0["r_safe"] == base.r_safe).all() and list(g0["W"]) == list(base.W)
        if c["level"] >= 2:      # a radius of its own per obstacle and group, a decoy in the absent entries
            for e in inp["groups"][1:]:
                assert len(set(e["r_safe"].tolist())) == no and (e["r_safe"] >= 1.6).all() and (e["r_safe"] <= 3.0).all()
            want = np.stack([np.where(inp["groups"][k]["mask"], inp["groups"][k]["r_safe"], inp["groups"][k]["r_safe"] + fk.DECOY_RADIUS) for k in inp["group"]])
            assert np.array_equal(inp["r_safe"], want)
        if c["level"] >= 3:
            assert (~inp["mask"][:, 0]).any()


@pytest.mark.parametrize("Bs", [1037, 1165])
def test_embedded_batch_keeps_the_case_and_every_filler_row_is_its_own(orc, Bs):
    """feature_kernel_cases.embed (the scheduled sweeps' batch): the judged rows are the case's bit for bit; in every feature array no filler row
    equals a judged row or another filler row, so a kernel that reads row `slot` for instance `inst` solves another problem; the arrays pass the
    host side of the setters.  Exempt from "every row its own" are the arrays of small integers: the offsets (0 .. 3; the yref rows they select
    differ) and the masks (n_obst bits, three values at two obstacles; the radii rows they go with differ), of which several values must occur"""
    import mpc_gpu
    import slack_schedule_cases as ss
    from mpc_gpu import pack_instance_bounds, pack_obstacle_mask
    pos = fk.positions(Bs)
    for c in (fk.cases_of("split", 1)[0], fk.cases_of("one", 2)[1], fk.cases_of("wide", 3)[0], fk.cases_of("split", 4)[0]):
        inp = fk.inputs(orc, c)
        alpha = ss.feature_problem(orc, c, "own")["alpha"] if c["level"] == 4 else None
        e = fk.embed(orc, inp, Bs, pos, alpha=alpha, with_P=c["level"] == 1)
        N, no = c["N"], c["no"]
        assert e["filler"].sum() == Bs - fk.B and not e["filler"][pos].any() and pos[0] == 0 and pos[-1] == Bs - 1
        for k in fk.EMBEDDED + (("P",) if c["level"] == 1 else ()):
            assert e[k].shape[0] == Bs and e[k].dtype == inp[k].dtype and np.array_equal(e[k][pos], inp[k]), k
        for k in inp["bounds"]:
            assert np.array_equal(e["bounds"][k][pos], inp["bounds"][k]), k
        if alpha is not None:
            assert np.array_equal(e["alpha"][pos], alpha) and np.isfinite(e["alpha"]).all() and (e["alpha"] >= 0).all() and (e["alpha"] <= 1e300).all()
        for k in fk.FEATURE_ARRAYS + ("x0", "goal", "obst", "noise"):
            if k == "alpha" and alpha is None:
                continue
            rows = fk.distinct_rows(e, k)
            assert len(np.unique(rows, axis=0)) == Bs - (fk.B - len(np.unique(rows[pos], axis=0))), k      # (judged rows of one group may be equal)
            assert not (rows[e["filler"]][:, None, :] == rows[pos][None, :, :]).all(axis=2).any(), k
        fill = e["filler"]
        assert set(e["offset"][fill].tolist()) == {0, 1, 2, 3}
        for b in np.nonzero(fill)[0][:50]:      # the decoy in front of the offset, the goal at and behind it
            o = e["offset"][b]
            assert np.array_equal(e["yref"][b, o:, :2], np.tile(e["goal"][b], (e["T"] - o, 1))) and np.array_equal(e["yref"][b, :o, :2], np.tile(e["goal"][b] + (5.0, -5.0), (o, 1)))
        idle = (e["ep_flags"] != 0) & fill
        assert 3 <= idle.sum() <= Bs // 50 and set(e["ep_flags"].tolist()) == {0, 1} and (e["x0"][fill, 3:] == 0).all()
        assert e["mask"].any(axis=1).all() and (e["mask"].all() if c["level"] < 3 else len(np.unique(e["mask"][fill], axis=0)) >= 3)
        r = np.where(e["mask"], e["r_safe"], e["r_safe"] - fk.DECOY_RADIUS)[fill]
        assert (r >= 1.6).all() and (r <= 3.0).all()
        for k, base in (("W", fk.IP["W"]), ("We", fk.IP["We"])):
            f = e[k][fill] / np.array(base)
            assert (f >= 0.5).all() and (f <= 3.0).all(), k
        # the host side of the setters: the packed words and table, every box with an interior
        words = pack_obstacle_mask(e["mask"])
        assert words.shape == (Bs,) and (words > 0).all() and (words < (1 << no)).all()
        t = pack_instance_bounds(mpc_gpu.default_config(N, no, 0.1 * N), Bs, **e["bounds"])
        assert t.shape == (Bs, 12) and np.isfinite(t).all() and (t[:, 0:2] < t[:, 2:4]).all() and (t[:, 4:8] < t[:, 8:12]).all()


def test_oracle_takes_per_obstacle_radii(orc):
    """oracle.obstacle_radii: equal radii are the config's radius bit for bit, one changed radius changes the solve, and nothing stays set behind the block"""
    N, no = 20, 3
    c = fk.cases_of("split", 2)[3]
    assert (c["N"], c["no"]) == (N, no)
    inp = fk.inputs(orc, c)
    cfg = orc.config(N, no, 0.1 * N)
    x0, goal, P = inp["x0"][2:6], inp["goal"][2:6], np.ascontiguousarray(inp["P"][2:6])
    X, U = (np.stack(v) for v in zip(*[orc.initial_guess(cfg, x) for x in x0]))
    plain = orc.rti_solve_batch(cfg, x0, P, goal, X, U)
    with orc.obstacle_radii(np.full(no, cfg.r_safe)):
        same = orc.rti_solve_batch(cfg, x0, P, goal, X, U)
    with orc.obstacle_radii([cfg.r_safe, cfg.r_safe, cfg.r_safe + 0.6]):
        other = orc.rti_solve_batch(cfg, x0, P, goal, X, U)
        cost = orc.cost(cfg, x0[0], P[0], goal[0], X[0], U[0])
        q = orc.export_qp(cfg, x0[0], P[0], goal[0], X[0], U[0])
    after = orc.rti_solve_batch(cfg, x0, P, goal, X, U)
    for k in ("X", "U", "cost", "status", "iters"):
        assert np.array_equal(plain[k], same[k]) and np.array_equal(plain[k], after[k]), k
    assert not np.array_equal(plain["X"], other["X"])
    # the third obstacle's rows of the exported QP moved by r^2 - (r + 0.6)^2, the others not at all; the cost went through the same radii
    q0 = orc.export_qp(cfg, x0[0], P[0], goal[0], X[0], U[0])
    d = (q["hs"] - q0["hs"]).reshape(-1, no)
    assert np.abs(d[:, :2]).max() == 0.0 and np.allclose(d[:, 2], cfg.r_safe ** 2 - (cfg.r_safe + 0.6) ** 2, rtol=1e-12, atol=0.0)
    assert cost >= orc.cost(cfg, x0[0], P[0], goal[0], X[0], U[0])
    with pytest.raises(ValueError):
        with orc.obstacle_radii(np.ones(33)):
            pass


def test_oracle_alone_converges_on_every_case(orc):
    """every non-idle instance, both solves, status 0; at level 3 and 4 an instance with an absent obstacle; at level 4 a bound of the group's own
    active in the first solve of at least a quarter of the instances of groups 1 to 3"""
    bad, seen = [], {}
    for c in fk.enumerate_cases():
        key = (c["N"], c["no"], c["level"])
        if key not in seen:         # (cases that differ in the lane mapping alone share their inputs)
            inp = fk.inputs(orc, c)
            res = fk.oracle_alone(orc, c, inp)
            ok = [0, 0]
            active = 0
            for k, (idx, cfg, first, second) in enumerate(res):
                live = inp["ep_flags"][idx] == 0
                ok[0] += int((first["status"][live] == 0).sum()); ok[1] += int((second["status"][live] == 0).sum())
                if c["level"] >= 4 and k >= 1:
                    active += sum(fk.bound_active(inp["groups"][k]["bounds"], c["N"], first["X"][i], first["U"][i]) for i in range(len(idx)))
            absent = int((~inp["mask"]).any(axis=1).sum())
            seen[key] = (ok, absent, active)
            print(f"ORACLE-ALONE N {c['N']} n_obst {c['no']} level {c['level']}: status 0 in {ok[0]} / {ok[1]} of {fk.B - 1} live instances "
                  f"(first / second solve); instances with an absent obstacle {absent}; own bound active {active} of 9")
        ok, absent, active = seen[key]
        if ok != [fk.B - 1, fk.B - 1]:
            bad.append((c["name"], "converged", ok))
        if c["level"] >= 3 and absent < 1:
            bad.append((c["name"], "no absent obstacle"))
        if c["level"] >= 4 and 4 * active < 9:
            bad.append((c["name"], "bounds inactive", active))
    print(f"ORACLE-ALONE {len(seen)} distinct inputs, {len(fk.enumerate_cases())} cases")
    assert not bad, bad
