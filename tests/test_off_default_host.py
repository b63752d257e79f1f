"""The off-default net without a GPU (off_default_cases.py).  The oracle is the reference of every GPU comparison
at dt != 0.1 and under an asymmetric arena, so it is pinned there on its own: the closed-form step against the collocation it stands for, the
linearisation against finite differences, the look-ahead against a numpy transcription of docs/PROBLEM.md, bit for bit.  The rows of the case table
are solved by the oracle alone and the counts of converged instances stored in the table are asserted, and the generators are what they claim."""
import numpy as np
import pytest

import off_default_cases as oc
from helpers import oracle_P, random_batch

STEPS = (0.05, 0.16, 0.25)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


def _converged(res):
    return tuple(int((o["status"] == 0).sum()) for _, _, o in res)


def _at_the_cap(cfg, res):
    return any(bool(((o["status"] != 0) & (o["iters"] >= cfg.qp_iter_max)).any()) for _, _, o in res)


# ---------------------------------------------------------------------------------------------------------------- the case table
@pytest.mark.parametrize("off", [False, True], ids=["default", "OFF"])
@pytest.mark.parametrize("row", oc.ROWS, ids=[r["id"] for r in oc.ROWS])
def test_oracle_alone_converges_as_the_table_says(orc, row, off):
    kw = oc.row_cfg(off)
    x0, goal, obst = oc.scaled_batch(row["B"], row["no"], row["seed"], kw.get("arena", oc.DEFAULT_ARENA))
    cfg = orc.config(row["N"], row["no"], row["Tf"], **kw)
    assert abs(cfg.Tf / cfg.N - 0.1) > 0.015                      # the point of the table
    res = oc.oracle_three_solves(orc, cfg, x0, oracle_P(orc, cfg, obst), goal)
    got = _converged(res)
    assert got == tuple(row["ok_off" if off else "ok_default"]), (row["id"], got)
    assert min(got) >= row["B"] - 1
    assert _at_the_cap(cfg, res) == (row["capped"] if off else False)
    if not off:
        assert max(int(o["iters"].max()) for _, _, o in res) <= 26


@pytest.mark.parametrize("sw", oc.SWITCHES)
@pytest.mark.parametrize("rid", oc.SWITCH_ROWS)
def test_switch_counts(orc, rid, sw):
    """one cold solve of the oracle alone per (row, switch): the stored count, and the pair is dropped exactly when fewer than B - 2 converge"""
    row = oc.ROW[rid]
    x0, goal, obst = oc.scaled_batch(row["B"], row["no"], row["seed"], oc.DEFAULT_ARENA)
    cfg = orc.config(row["N"], row["no"], row["Tf"], **{sw: oc.SWITCH_VALUE[sw]})
    _, _, o = oc.oracle_three_solves(orc, cfg, x0, oracle_P(orc, cfg, obst), goal)[0]
    n = int((o["status"] == 0).sum())
    assert n == oc.SWITCH_OK[rid][sw], (rid, sw, n)
    assert (n < row["B"] - 2) == ((rid, sw) in oc.SWITCH_DROPPED), (rid, sw, n)


def test_dropped_pairs_are_what_the_counts_say():
    dropped = tuple((r, sw) for r in oc.SWITCH_ROWS for sw in oc.SWITCHES if oc.SWITCH_OK[r][sw] < oc.ROW[r]["B"] - 2)
    assert dropped == tuple(oc.SWITCH_DROPPED)
    assert len(oc.switch_cases()) == len(oc.SWITCH_ROWS) * len(oc.SWITCHES) - len(oc.SWITCH_DROPPED)
    assert all(sw == "soft_h" for _, sw in oc.SWITCH_DROPPED)


@pytest.mark.parametrize("rid", sorted(oc.FEATURE_OK))
def test_feature_level_counts(orc, rid):
    row = oc.ROW[rid]
    kw = dict(oc.OFF, **oc.IP)
    x0, goal, obst = oc.scaled_batch(row["B"], row["no"], row["seed"], kw["arena"])
    cfg = orc.config(row["N"], row["no"], row["Tf"], **kw)
    got = _converged(oc.oracle_three_solves(orc, cfg, x0, oracle_P(orc, cfg, obst), goal))
    assert got == tuple(oc.FEATURE_OK[rid]) and min(got) >= row["B"] - 1, (rid, got)


# ---------------------------------------------------------------------------------------------------------------- the oracle at dt != 0.1
@pytest.mark.parametrize("dt", STEPS)
def test_closed_form_equals_gl4_collocation_off_the_default_step(orc, dt):
    """test_oracle_math.py::test_closed_form_equals_gl4_collocation at other steps, to its bound"""
    rng = np.random.default_rng(int(1000 * dt))
    for _ in range(300):
        x = np.array([*rng.uniform(-7, 7, 2), rng.uniform(-6, 6), *rng.uniform(-10, 10, 2)])
        u = rng.uniform(-8, 8, 2)
        for p, q in zip(orc.dynamics(x, u, dt), orc.dynamics_collocation(x, u, dt, 3)):
            assert np.abs(p - q).max() < 1e-13, dt


@pytest.mark.parametrize("dt", STEPS)
def test_linearize_against_finite_differences_off_the_default_step(orc, dt):
    """A, B and the defect b of orc.linearize (which takes its step from the config, Tf / N) against central differences of orc.dynamics at that step"""
    N, no = 6, 2
    cfg = orc.config(N, no, dt * N)
    x0, goal, obst = random_batch(1, no, seed=2)
    rng = np.random.default_rng(7)
    X = np.column_stack([rng.uniform(-7, 7, (N + 1, 2)), rng.uniform(-3, 3, N + 1), rng.uniform(-5, 5, (N + 1, 2))])
    U = rng.uniform(-8, 8, (N, 2))
    L = orc.linearize(cfg, x0[0], oracle_P(orc, cfg, obst)[0], goal[0], X, U)
    h = cfg.Tf / cfg.N
    for i in range(N):
        f0 = orc.dynamics(X[i], U[i], h)[0]
        assert np.abs(L["b"][i] - (f0 - X[i + 1])).max() < 1e-13
        for k in range(5):
            e = np.zeros(5); e[k] = 1e-6
            fd = (orc.dynamics(X[i] + e, U[i], h)[0] - orc.dynamics(X[i] - e, U[i], h)[0]) / 2e-6
            assert np.abs(fd - L["A"][i][:, k]).max() < 1e-8, (dt, i, k)
        for k in range(2):
            e = np.zeros(2); e[k] = 1e-6
            fd = (orc.dynamics(X[i], U[i] + e, h)[0] - orc.dynamics(X[i], U[i] - e, h)[0]) / 2e-6
            assert np.abs(fd - L["B"][i][:, k]).max() < 1e-8, (dt, i, k)
    # the entries that are the step itself: psi' = psi + dt omega + dt^2 / 2 u_alpha, v' = v + dt u_a
    assert np.allclose(L["A"][:, 2, 4], h, rtol=1e-15) and np.allclose(L["B"][:, 3, 0], h, rtol=1e-15) and np.allclose(L["B"][:, 2, 1], 0.5 * h * h, rtol=1e-14)


@pytest.mark.parametrize("bug", [1, 0], ids=["D1", "fixed"])
@pytest.mark.parametrize("dt", [0.05, 0.07, 0.16, 0.25])
@pytest.mark.parametrize("N", [5, 20, 21, 50])
def test_lookahead_under_an_asymmetric_arena_is_the_transcription(orc, N, dt, bug):
    """orc.predict_params under OFF's arena against off_default_cases.lookahead (written from docs/PROBLEM.md), bit for bit, on the wall cases"""
    no, B = 3, 6
    arena = oc.OFF["arena"]
    _, _, obst, hits = oc.wall_cases(B, no, 60 + N, arena, dt)
    cfg = orc.config(N, no, dt * N, arena=arena, bug_compat_predict=bug)
    step = cfg.Tf / cfg.N                       # (what the oracle divides out: dt to an ulp)
    reflected = 0
    for b in range(B):
        P = orc.predict_params(cfg, obst[b])
        for j in range(no):
            want, first = oc.lookahead(arena, obst[b, j], N, step, bug_compat=bool(bug))
            assert np.array_equal(P[:, j], want), (b, j)
            reflected += sum(1 for f in first if f)
    assert reflected >= sum(1 for h in hits if h["stage"] <= N and (h["motion"] == "both" or not bug)) >= 5


@pytest.mark.parametrize("dt", [0.05, 0.07, 0.16, 0.25])
def test_ground_truth_motion_under_an_asymmetric_arena_is_the_transcription(orc, dt):
    """orc.obstacle_step without noise (the ground-truth motion: x moves with vx) under OFF's arena, eight steps running, against stage 1 of
    off_default_cases.lookahead with the defect D1 off, bit for bit, on the wall cases; instance 3's x reflects at xmin in this motion alone"""
    no, B, N = 3, 6, 20
    arena = oc.OFF["arena"]
    _, _, obst, hits = oc.wall_cases(B, no, 77, arena, dt)
    cfg = orc.config(N, no, dt * N, arena=arena)
    step = cfg.Tf / cfg.N
    turned = set()
    for b in range(B):
        for j in range(no):
            st = obst[b, j].copy()
            for k in range(1, 9):
                traj, first = oc.lookahead(arena, st, 1, step, bug_compat=False)
                nxt = orc.obstacle_step(cfg, st, step)
                assert np.array_equal(nxt[:2], traj[1]), (b, j, k)
                for a in (0, 1):
                    assert nxt[2 + a] == (-st[2 + a] if first[a] else st[2 + a]), (b, j, k, a)
                    if first[a]:
                        turned.add((b, j, a, k))
                st = nxt
    for h in hits:      # every stated first reflection happens, in its stage, in the oracle's ground-truth motion
        assert (h["b"], h["j"], h["axis"], h["stage"]) in turned, h
        assert not any(t[:3] == (h["b"], h["j"], h["axis"]) and t[3] < h["stage"] for t in turned), h


# ---------------------------------------------------------------------------------------------------------------- the generators
@pytest.mark.parametrize("B,no,seed", [(16, 3, 31), (8, 32, 37), (8, 1, 5)])
def test_scaled_batch_is_random_batch_at_the_default_arena(B, no, seed):
    for a, b in zip(oc.scaled_batch(B, no, seed, oc.DEFAULT_ARENA), random_batch(B, no, seed=seed)):
        assert np.array_equal(a, b)
    x0, goal, obst = oc.scaled_batch(B, no, seed, oc.OFF["arena"])
    r0, rg, ro = random_batch(B, no, seed=seed)
    xmin, xmax, ymin, ymax = oc.OFF["arena"]
    assert np.allclose(x0[:, 0], 1.25 + r0[:, 0] * 15.5 / 16, rtol=1e-15) and np.allclose(goal[:, 1], -1.25 + rg[:, 1] * 16.5 / 16, rtol=1e-15)
    assert np.array_equal(obst[:, :, 2:], ro[:, :, 2:]) and np.array_equal(x0[:, 2:], r0[:, 2:])
    assert (obst[:, :, 0] > xmin).all() and (obst[:, :, 0] < xmax).all() and (obst[:, :, 1] > ymin).all() and (obst[:, :, 1] < ymax).all()


@pytest.mark.parametrize("arena", [oc.OFF["arena"], oc.DEFAULT_ARENA], ids=["OFF", "default"])
@pytest.mark.parametrize("dt", [0.05, 0.07, 0.08, 0.1, 0.15, 0.16, 0.25])
@pytest.mark.parametrize("no", [1, 3, 32])
def test_wall_cases_reflect_where_they_say(arena, dt, no):
    N = 21
    x0, goal, obst, hits = oc.wall_cases(8, no, 9, arena, dt)
    wall_value = dict(zip(("xmin", "xmax", "ymin", "ymax"), arena))
    assert {h["wall"] for h in hits} == {"xmin", "xmax", "ymin", "ymax"}
    assert {h["stage"] for h in hits} >= ({1, 2, 3, 7} if no >= 2 else {1, 2, 3})
    for h in hits:
        st = obst[h["b"], h["j"]]
        for bug in (True, False):
            traj, first = oc.lookahead(arena, st, N, dt, bug_compat=bug)
            stated = h["motion"] == "both" or not bug
            assert (first[h["axis"]] == h["stage"]) == stated, (h, bug, first)
            if stated:
                # the wall lies between the positions either side of the reflection, and the coordinate turns round there
                k, a, w = h["stage"], h["axis"], wall_value[h["wall"]]
                up = h["wall"] in ("xmax", "ymax")
                assert ((traj[:, a] <= w) if up else (traj[:, a] >= w)).all()
                before = np.diff(traj[:k, a]); after = traj[k + 1, a] - traj[k, a]
                assert ((before > 0) if up else (before < 0)).all() and ((after < 0) if up else (after > 0))
    assert obst[1, 0, 0] == arena[1]                                 # exactly on the wall
    b2 = [h for h in hits if h["b"] == 2]
    assert len(b2) == 2 and b2[0]["stage"] != b2[1]["stage"]         # the corner: two coordinates, two stages
