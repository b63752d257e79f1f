"""The slack-schedule sweep without a GPU: the oracle's QP export with a schedule (what helpers.adjudicate settles an
instance beyond the tolerance against), the recipe of slack_schedule_cases.schedule, and -- on the oracle alone, for every problem the GPU tests
run -- the conditions that make the GPU comparison mean something: every live instance converges from the cold guess and from the result, and at
least three instances move by more than 1e-4 when the terminal weight is zeroed, when the hole inside the horizon is filled, and when an instance
is solved with its neighbour's row."""
import numpy as np
import pytest

import feature_kernel_cases as fk
import slack_schedule_cases as ss
import sqp_cases as sc
from helpers import adjudicate, oracle_P, oracle_guess, qp_merit, random_batch


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


def _one(orc, N=12, no=3, seed=5, **kw):
    x0, goal, obst = random_batch(4, no, seed=seed)
    cfg = orc.config(N, no, 0.1 * N, **kw)
    P = oracle_P(orc, cfg, obst)
    X, U = oracle_guess(orc, cfg, x0)
    return cfg, x0, goal, P, X, U


def test_export_with_the_builtin_schedule_passed_back_is_the_plain_export(orc):
    cfg, x0, goal, P, X, U = _one(orc)
    for b in range(4):
        own = orc.slack_alpha(cfg, x0[b], goal[b])
        a, q = orc.export_qp(cfg, x0[b], P[b], goal[b], X[b], U[b]), orc.export_qp(cfg, x0[b], P[b], goal[b], X[b], U[b], alpha=own)
        assert set(a) == set(q)
        for k in a:
            assert np.array_equal(a[k], q[k]), k
    with pytest.raises(ValueError):
        orc.export_qp(cfg, x0[0], P[0], goal[0], X[0], U[0], alpha=np.ones(cfg.N))


@pytest.mark.parametrize("scale_dt", [1, 0])
def test_export_with_a_sparse_schedule_is_the_direct_construction(orc, scale_dt):
    """soft rows exist at the stages 1 .. N with a positive weight and nowhere else, n_obst per stage, stage by stage; zs = Zs = the weight, times dt
    below the terminal stage when slack_scale_dt, unscaled on the terminal stage; each row is the obstacle constraint linearised at that stage"""
    N, no = 12, 3
    cfg, x0, goal, P, X, U = _one(orc, N, no, slack_scale_dt=scale_dt)
    dt = cfg.Tf / N
    alpha = np.zeros(N + 1)
    alpha[[0, 2, 3, 7, N]] = [9.0, 40.0, 5e5, 1e3, 77.0]        # (stage 0 has no rows whatever its weight)
    for b in range(4):
        q = orc.export_qp(cfg, x0[b], P[b], goal[b], X[b], U[b], alpha=alpha)
        lin = orc.linearize(cfg, x0[b], P[b], goal[b], X[b], U[b])
        stages = [i for i in range(1, N + 1) if alpha[i] > 0]
        assert len(q["hs"]) == no * len(stages) == q["Cs"].shape[0] == len(q["zs"]) == len(q["Zs"])
        want_z = np.repeat([alpha[i] * (dt if scale_dt and i < N else 1.0) for i in stages], no)
        assert np.array_equal(q["zs"], want_z) and np.array_equal(q["Zs"], want_z)
        assert q["zs"][-1] == 77.0
        Cs = np.zeros((no * len(stages), 7 * N))
        for k, i in enumerate(stages):
            for j in range(no):
                Cs[k * no + j, 7 * (i - 1) + 2: 7 * (i - 1) + 4] = lin["dh"][i, j]
        assert np.array_equal(q["Cs"], Cs)
        assert np.array_equal(q["hs"], np.concatenate([lin["h"][i] for i in stages]))
        plain = orc.export_qp(cfg, x0[b], P[b], goal[b], X[b], U[b])
        for k in ("H", "g", "Aeq", "beq", "lb", "ub"):            # the schedule touches the soft rows alone
            assert np.array_equal(q[k], plain[k]), k
    q = orc.export_qp(cfg, x0[0], P[0], goal[0], X[0], U[0], alpha=np.zeros(N + 1))
    assert len(q["hs"]) == 0


def test_adjudication_takes_the_schedule(orc):
    """the oracle's own step is the exact solution of the QP exported with ITS schedule (adjudicate: distance below the cap), and not of the QP of
    another schedule; qp_merit sees the same"""
    p = ss.around_problem(orc, "split")
    cfg, x0, goal, P, X, U, alpha = p["cfg"], p["x0"], p["goal"], p["groups"][0]["P"], p["X0"], p["U0"], p["alpha"]
    far = 0
    for b in range(p["B"]):
        r = orc.rti_solve(cfg, x0[b], P[b], goal[b], X[b], U[b], alpha=alpha[b])
        assert r["status"] == 0
        a = adjudicate(orc, cfg, x0[b], P[b], goal[b], X[b], U[b], r["X"], r["U"], r["X"], r["U"], alpha=alpha[b])
        assert a["passed"] and a["kind"] == "exact" and a["d_gpu"] <= 1e-6, a
        plain = adjudicate(orc, cfg, x0[b], P[b], goal[b], X[b], U[b], r["X"], r["U"], r["X"], r["U"])
        far += plain["kind"] == "exact" and plain["d_gpu"] > 1e-4
        f, eq, bnd = qp_merit(orc, cfg, x0[b], P[b], goal[b], X[b], U[b], r["X"], r["U"], alpha=alpha[b])
        assert eq <= 1e-7 and bnd <= 1e-7 and np.isfinite(f)
    assert far >= 1


def test_batch_solve_with_schedules_is_the_single_solves(orc):
    cfg, x0, goal, P, X, U = _one(orc, 12, 3, seed=9)
    alpha = ss.schedule(12, 8, 3, builtin=np.zeros(13))[:4]
    o = orc.rti_solve_batch(cfg, x0, P, goal, X, U, alpha=alpha)
    for b in range(4):
        r = orc.rti_solve(cfg, x0[b], P[b], goal[b], X[b], U[b], alpha=alpha[b])
        assert np.array_equal(o["X"][b], r["X"]) and np.array_equal(o["U"][b], r["U"]) and o["status"][b] == r["status"] and o["iters"][b] == r["iters"]
        assert o["cost"][b] == r["cost"] and np.array_equal(o["u0"][b], r["u0"])
    with pytest.raises(ValueError):
        orc.rti_solve_batch(cfg, x0, P, goal, X, U, alpha=alpha[:3])


@pytest.mark.parametrize("N,B", [(10, 12), (20, 37), (31, 12), (50, 12)])
def test_the_recipe(N, B):
    own = np.linspace(3e4, 0.0, N + 1)
    a = ss.schedule(N, B, 1, builtin=own)
    assert a.shape == (B, N + 1) and np.isnan(ss.schedule(N, B, 1)[ss.BUILTIN_ROW]).all()
    special = [ss.ZERO_ROW, ss.TERMINAL_ROW, ss.BUILTIN_ROW]
    plain = np.array([b for b in range(B) if b not in special])
    assert len({r.tobytes() for r in a}) == B                                   # every row different
    zero = [N // 3, N // 3 + 1, N - 1]
    assert (a[plain][:, zero] == 0).all() and (a[plain, N] > 0).all()
    assert (a[plain[plain % 4 == 0], 1] == 0).all() and (a[plain[plain % 4 != 0], 1] > 0).all()
    rest = np.ones(N + 1, bool); rest[zero] = False; rest[1] = False
    assert (a[plain][:, rest] >= 1e1).all() and (a[plain][:, rest] <= 1e6).all()
    assert (a[ss.ZERO_ROW] == 0).all() and (a[ss.TERMINAL_ROW, :N] == 0).all() and a[ss.TERMINAL_ROW, N] > 0
    assert np.array_equal(a[ss.BUILTIN_ROW], own)
    assert np.array_equal(a, ss.schedule(N, B, 1, builtin=own)) and not np.array_equal(a, ss.schedule(N, B, 2, builtin=own))
    h = ss.hole_filled(a)
    assert (h[plain][:, [N // 3, N // 3 + 1]] > 0).all() and (ss.without_terminal(a)[:, N] == 0).all() and np.array_equal(ss.next_row(a)[0], a[1])


_PROBLEMS = {}


def _problems(orc):
    if not _PROBLEMS:
        _PROBLEMS.update(ss.every_problem(orc))
    return _PROBLEMS


def test_the_problems_are_the_cases_the_gpu_tests_run(orc):
    probs = _problems(orc)
    kinds = [k[0] for k in probs]
    assert kinds.count("level0") == len(ss.LEVEL0_SHAPES) == 24 and kinds.count("sqp") == len(sc.CASES) == 11
    assert {(c["N"], c["no"], c["level"]) for c in fk.enumerate_cases()} == {k[1:] for k in probs if k[0] == "feature"}
    for key, p in probs.items():
        a = p["alpha"]
        assert a.shape == (p["B"], p["N"] + 1) and np.isfinite(a).all() and (a >= 0).all()
        own = orc.slack_alpha(next(g["cfg"] for g in p["groups"] if ss.BUILTIN_ROW in g["idx"]), p["x0"][ss.BUILTIN_ROW], p["goal"][ss.BUILTIN_ROW])
        assert np.array_equal(a[ss.BUILTIN_ROW], own), key
        arena = [float(v) for v in p["groups"][0]["cfg"].arena]
        ob = p["inp"]["obst"] if "inp" in p else p["obst"]
        assert (ob[:, :, 0] >= arena[0]).all() and (ob[:, :, 0] <= arena[1]).all() and (ob[:, :, 1] >= arena[2]).all() and (ob[:, :, 1] <= arena[3]).all(), key
        assert sorted(np.concatenate([g["idx"] for g in p["groups"]]).tolist()) == list(range(p["B"])), key
    # the feature cases keep everything but the obstacles of their own inputs; the SQP cases likewise
    case = fk.enumerate_cases()[40]
    mine, theirs = ss.feature_problem(orc, case)["inp"], fk.inputs(orc, case)
    for k in theirs:
        if k not in ("obst", "P", "groups", "bounds"):
            assert np.array_equal(mine[k], theirs[k], equal_nan=True), k
    assert not np.array_equal(mine["obst"], theirs["obst"]) and np.array_equal(mine["obst"][:, :, 2:], theirs["obst"][:, :, 2:])


def test_every_problem_meets_the_conditions_on_the_oracle_alone(orc):
    bad = []
    for key, p in _problems(orc).items():
        hard = not p["groups"][0]["cfg"].soft_h
        c = ss.oracle_conditions(orc, p)
        line = (f"SLACK-SCHEDULE-HOST {key} seed {p['seed']}: live {int(p['live'].sum())} cold_ok {c['cold_ok']} warm_ok {c['warm_ok']} iterations <= {c['iters_max']} "
                f"moved: terminal {c['terminal']} hole {c['hole']} row {c['row']} terminal weight x dt {c['scaled']}")
        print(line)
        if hard:
            # soft_h = 0: the rows are hard at every stage >= 1 whatever the schedule -- the oracle's result does not depend on it (bit for bit), some of
            # the linearised problems are infeasible (status 4) and some are not
            o = ss.oracle_solve(orc, p, np.zeros_like(p["alpha"]))
            same = all(np.array_equal(o[k], c["first"][k]) for k in ("X", "U", "status", "iters"))      # (the reported cost keeps the schedule's penalty)
            st = c["first"]["status"]
            if not (same and (st == 0).sum() >= 3 and (st == 4).sum() >= 1 and np.isin(st, (0, 2, 4)).all()):
                bad.append(line + f" hard rows: same {same} status {st.tolist()}")
            continue
        counts = [c["terminal"], c["hole"], c["row"]]
        if ss.slack_scale(p) != 1.0:        # (slack_scale_dt = 0: no stage's weight is scaled, the terminal one is like the others by construction)
            counts.append(c["scaled"])
        if not (c["cold_ok"] and c["warm_ok"] and min(counts) >= ss.MIN_MOVED):
            bad.append(line)
    assert not bad, "\n".join(bad)


def test_the_cases_on_their_own_inputs_converge(orc):
    """the second world of the GPU sweeps of levels 1 to 5: the cases' own inputs, untouched, with the schedule on top -- every live instance converges
    (how many instances feel the schedule there is printed, not asked: in batches of twelve with few obstacles it is fewer than three whatever the seed)"""
    for case in fk.enumerate_cases():
        mine, theirs = ss.feature_problem(orc, case, "own")["inp"], fk.inputs(orc, case)
        assert all(np.array_equal(mine[k], theirs[k], equal_nan=True) for k in ("x0", "goal", "obst", "P", "noise", "yref", "offset", "mask", "W", "We", "r_safe"))
    for key, p in ss.own_world_problems(orc).items():
        if key[0] != "feature-own":
            continue
        c = ss.oracle_conditions(orc, p)
        print(f"SLACK-SCHEDULE-HOST {key}: cold_ok {c['cold_ok']} moved: terminal {c['terminal']} hole {c['hole']} row {c['row']} terminal weight x dt {c['scaled']}")
        assert c["cold_ok"], key


@pytest.mark.parametrize("world", ss.WORLDS)
@pytest.mark.parametrize("cid", sc.IDS)
def test_the_three_fold_sequence_converges(orc, cid, world):
    """level 5 runs set_sqp(3, 0): every finite instance converges in each of the three iterations, the NaN instance fails at once"""
    c = sc.case(cid)
    p = ss.sqp_problem(orc, c, world)
    o = sc.oracle_sequence(orc, c, step_tol=0.0, max_iter=3, alpha=p["alpha"], P=p["inp"]["P"])
    fin = sc.finite_instances()
    assert (o["statuses"][fin] == 0).all() and (o["sqp_iters"][fin] == 3).all(), o["statuses"]
    assert o["status"][sc.NAN_INSTANCE] == 4 and o["sqp_iters"][sc.NAN_INSTANCE] == 1
    plain = sc.oracle_sequence(orc, c, step_tol=0.0, max_iter=3, P=p["inp"]["P"])
    assert world == "own" or (np.abs(o["X"][fin] - plain["X"][fin]).max(axis=(1, 2)) > ss.MOVED).sum() >= ss.MIN_MOVED
