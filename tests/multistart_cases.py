"""Test infrastructure of the multi-start solve (mpc_seed_guesses_dev, mpc_select_best_dev, mpc_gpu.MultiStartMpc; test_multistart_host.py,
test_gpu_multistart.py): three scenes with an obstacle on the line from robot to goal, the lateral offsets, numpy restatements of the guess family and
of the selection rule as include/mpc_gpu.h words them, and the oracle-side group solve.  Imports without torch or a GPU; the oracle is passed in.  No
test functions here.

Several iterations per candidate follow the stop rule of mpc_set_sqp as tests/sqp_cases.py states and implements it (oracle_sequence): for k = 1, 2, ...
solve once from the current iterate; end behind iteration k when its status is 4 (the iterate stays that of iteration k - 1), or k == max_iter, or the
applied step has max-norm <= step_tol.  oracle_sequence itself is written over that module's own twelve-instance cases, so the loop is restated here for
one instance (`sequence`) with sqp_cases.step_norm as its norm; step_tol is 0 throughout (an instance stops early only on a status 4)."""
import numpy as np

from sqp_cases import step_norm

NO = 3
OFFSETS = (0.0, 2.5, -2.5, 5.0, -5.0)
K = len(OFFSETS)

# x0 = [x, y, psi, v, omega], goal = [x, y], obst rows = [x, y, vx, vy]
SCENES = {
    "A": dict(x0=[-5.0, 0.0, 0.0, 0.0, 0.0], goal=[5.0, 0.0], obst=[[0.0, 0.2, 0.0, 0.0], [2.0, -3.0, 0.0, 0.5], [-2.0, 3.0, 0.3, 0.0]]),
    "B": dict(x0=[-5.0, -5.0, 0.7, 0.0, 0.0], goal=[5.0, 5.0], obst=[[0.0, 0.0, 0.0, 0.0], [1.5, -1.5, -0.5, 0.5], [-2.0, 3.0, 0.3, 0.0]]),
    "C": dict(x0=[-3.0, 0.0, 0.0, 1.0, 0.0], goal=[4.0, 1.0], obst=[[0.0, -0.3, 0.0, 0.0], [0.5, 2.5, 0.0, -0.5], [-6.0, -6.0, 0.0, 0.0]]),
}

# the parity scenes: (scene, N, Tf, SQP iterations per launch)
PARITY = [("A", 20, 2.0, 1), ("B", 20, 2.0, 1), ("C", 20, 2.0, 1), ("A", 20, 2.0, 4), ("B", 20, 2.0, 4), ("C", 20, 2.0, 4), ("B", 50, 5.0, 4), ("C", 50, 5.0, 4)]
PARITY_IDS = [f"{s}-N{N}-it{it}" for s, N, Tf, it in PARITY]

# the closed loop in lockstep: (scene, incumbent margin), LOCKSTEP_STEPS control steps each at N = 20, Tf = 2, one RTI iteration per step
LOCKSTEP = [("C", 0.0), ("B", 0.0), ("B", 0.1)]
LOCKSTEP_IDS = [f"{s}-m{m}" for s, m in LOCKSTEP]
LOCKSTEP_STEPS = 6
LOCKSTEP_N, LOCKSTEP_TF = 20, 2.0

MIN_GAP = 1e-4      # relative cost gap between winner and runner-up below which a scene is not a parity scene (the cost parity tolerance is 1e-8)


def scene(name):
    s = SCENES[name]
    return np.array(s["x0"], dtype=np.float64), np.array(s["goal"], dtype=np.float64), np.array(s["obst"], dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------- the guess family
def guess(x0, goal, a, N):
    """the iterate of ONE member with lateral offset a: X (N + 1, 5), U (N, 2)"""
    x0, goal = np.asarray(x0, dtype=np.float64), np.asarray(goal, dtype=np.float64)
    X, U = np.zeros((N + 1, 5)), np.zeros((N, 2))
    d = goal - x0[:2]
    L = np.sqrt(d[0] * d[0] + d[1] * d[1])
    if L < 1e-9:                                  # the plain reset guess: [x, y, psi, 0, 0] at every stage
        X[:, :3] = x0[:3]
        return X, U
    with np.errstate(invalid="ignore"):
        t = d / L
        n = np.array([-t[1], t[0]])
        s = np.arange(N + 1) / N
        sn, cs = np.sin(np.pi * s), np.cos(np.pi * s)
        X[:, 0] = x0[0] + s * d[0] + a * sn * n[0]
        X[:, 1] = x0[1] + s * d[1] + a * sn * n[1]
        e = np.arctan2(d[1] + a * np.pi * cs * n[1], d[0] + a * np.pi * cs * n[0]) - x0[2]
        X[:, 2] = x0[2] + (e - 2.0 * np.pi * np.rint(e / (2.0 * np.pi)))
    X[0] = x0
    return X, U


def guesses(x0, goal, offsets, N):
    """the K iterates of one group: X (K, N + 1, 5), U (K, N, 2)"""
    Xs, Us = zip(*[guess(x0, goal, a, N) for a in offsets])
    return np.stack(Xs), np.stack(Us)


# ---------------------------------------------------------------------------------------------------------------- the selection rule
def eligible(cost, status):
    cost, status = np.asarray(cost, dtype=np.float64), np.asarray(status)
    return ((status == 0) | (status == 2)) & np.isfinite(cost)


def select(cost, status, margin=0.0):
    """one group (K,): (winner, best_cost) -- the eligible member of least cost, ties to the lowest index; with margin m > 0 an eligible member 0 stays
    unless the challenger costs less than (1 - m) cost[0]; (-1, +inf) when no member is eligible"""
    cost = np.asarray(cost, dtype=np.float64)
    ok = eligible(cost, status)
    w = -1
    for k in range(len(cost)):
        if ok[k] and (w < 0 or cost[k] < cost[w]):
            w = k
    if w < 0:
        return -1, np.inf
    if margin > 0.0 and ok[0] and w != 0 and not (cost[w] < (1.0 - margin) * cost[0]):
        w = 0
    return w, float(cost[w])


def select_groups(cost, status, margin=0.0, u0=None):
    """tables (G, K): winner (G,) int32, best_cost (G,), and with u0 (G, K, 2) best_u0 (G, 2) -- (0, 0) for a group without a winner"""
    cost, status = np.asarray(cost, dtype=np.float64), np.asarray(status)
    G = cost.shape[0]
    w, c = zip(*[select(cost[g], status[g], margin) for g in range(G)])
    w, c = np.array(w, np.int32), np.array(c, np.float64)
    if u0 is None:
        return w, c
    b = np.zeros((G, 2))
    for g in range(G):
        if w[g] >= 0:
            b[g] = np.asarray(u0)[g, w[g]]
    return w, c, b


def gap(cost, status, margin=0.0):
    """how far one group's selection is from going the other way, as a relative cost gap: between the least eligible cost and the next one, and -- where
    the margin decides, an eligible member 0 that is not the least -- between the least cost and (1 - m) cost[0] (inf with fewer than two eligible members)"""
    cost = np.asarray(cost, dtype=np.float64)
    w, c = select(cost, status, 0.0)
    ok = eligible(cost, status)
    others = [cost[k] for k in range(len(cost)) if k != w and ok[k]]
    if w < 0 or not others:
        return np.inf
    rel = lambda a, b: float(abs(a - b) / max(abs(a), abs(b)))
    g = rel(min(others), c)
    if margin > 0.0 and ok[0] and w != 0:
        g = min(g, rel(c, (1.0 - margin) * cost[0]))
    return g


# hand-made tables, (name, cost (K,), status (K,), margin, winner): what both the numpy rule and the kernel must answer
NAN, INF = float("nan"), float("inf")
HAND = [
    ("plain", [5.0, 3.0, 4.0, 9.0, 7.0], [0, 0, 0, 0, 0], 0.0, 1),
    ("tie to the lowest", [5.0, 3.0, 3.0, 9.0, 3.0], [0, 0, 0, 0, 0], 0.0, 1),
    ("tie with member 0", [3.0, 3.0, 4.0, 9.0, 3.0], [0, 2, 0, 0, 0], 0.0, 0),
    ("signed zeros tie", [0.0, -0.0, 4.0, 9.0, 3.0], [0, 0, 0, 0, 0], 0.0, 0),
    ("NaN is not eligible", [5.0, NAN, 4.0, 9.0, 7.0], [0, 0, 0, 0, 0], 0.0, 2),
    ("-inf is not eligible", [5.0, -INF, 4.0, 9.0, 7.0], [0, 0, 0, 0, 0], 0.0, 2),
    ("+inf is not eligible", [INF, INF, INF, 9.0, INF], [0, 0, 0, 2, 0], 0.0, 3),
    ("status 4 is not eligible", [5.0, 1.0, 4.0, 9.0, 7.0], [0, 4, 0, 0, 0], 0.0, 2),
    ("status 2 is eligible", [5.0, 1.0, 4.0, 9.0, 7.0], [0, 2, 0, 0, 0], 0.0, 1),
    ("an unknown status is not eligible", [5.0, 1.0, 4.0, 9.0, 7.0], [0, 3, 0, 1, -1], 0.0, 2),
    ("negative costs", [-1.0, -3.0, -2.0, 9.0, 7.0], [0, 0, 0, 0, 0], 0.0, 1),
    ("no eligible member", [NAN, 1.0, INF, -INF, 2.0], [0, 4, 0, 0, 4], 0.0, -1),
    ("no eligible member, margin", [NAN, 1.0, INF, -INF, 2.0], [0, 4, 0, 0, 4], 0.25, -1),
    ("margin kept", [10.0, 9.5, 12.0, 9.1, 11.0], [0, 0, 0, 0, 0], 0.1, 0),
    ("margin kept at the bound", [10.0, 7.5, 12.0, 9.5, 11.0], [0, 0, 0, 0, 0], 0.25, 0),
    ("margin beaten", [10.0, 9.5, 12.0, 8.9, 11.0], [0, 0, 0, 0, 0], 0.1, 3),
    ("margin, member 0 failed", [10.0, 9.5, 12.0, 9.6, 11.0], [4, 0, 0, 0, 0], 0.1, 1),
    ("margin, member 0 not finite", [NAN, 9.5, 12.0, 9.6, 11.0], [0, 0, 0, 0, 0], 0.1, 1),
    ("margin, member 0 is the least", [8.0, 9.5, 12.0, 9.6, 11.0], [0, 0, 0, 0, 0], 0.1, 0),
    ("last member", [5.0, 3.0, 4.0, 9.0, 1.0], [0, 0, 0, 0, 2], 0.0, 4),
]


def hand_table(Kt):
    """the hand-made cases as tables of Kt members per group: the five hand-made members, cut to Kt or padded with members that cost more (the last one least of them)
    and, every second one, a failed member that would cost less.  Returns a list of (margin, cost (G, Kt), status (G, Kt)) -- one table per margin in HAND."""
    out = {}
    for name, cost, status, margin, _ in HAND:
        c, s = list(cost[:Kt]), list(status[:Kt])
        for k in range(len(c), Kt):
            c.append(200.0 - k if k % 2 else -50.0 - k); s.append(0 if k % 2 else 4)
        out.setdefault(margin, []).append((c, s))
    return [(m, np.array([r[0] for r in rows], np.float64), np.array([r[1] for r in rows], np.int32)) for m, rows in out.items()]


# ---------------------------------------------------------------------------------------------------------------- the oracle side
def sequence(orc, cfg, x0, P, goal, X, U, max_iter, step_tol=0.0):
    """one instance: max_iter RTI iterations from (X, U) under mpc_set_sqp's stop rule (this module's docstring).  Returns the last solve's dict with
    X, U = the final iterate, iters = the sum, sqp_iters = the iterations run, iterates = the (X, U) in front of every iteration run"""
    X, U = X.copy(), U.copy()
    out = dict(iters=0, sqp_iters=0, iterates=[])
    for k in range(1, max_iter + 1):
        out["iterates"].append((X.copy(), U.copy()))
        r = orc.rti_solve(cfg, x0, P, goal, X, U)
        out["iters"] += r["iters"]; out["sqp_iters"] = k
        out.update(status=r["status"], u0=r["u0"], cost=r["cost"])
        if r["status"] == 4:
            break
        nrm = step_norm(X, U, r["X"], r["U"])
        X, U = r["X"], r["U"]
        if nrm <= step_tol:
            break
    out["X"], out["U"] = X, U
    return out


def group_solve(orc, cfg, x0, obst, goal, X, U, max_iter=1, margin=0.0):
    """the oracle's group solve from given member iterates X (K, N + 1, 5), U (K, N, 2): per candidate `sequence` on the oracle's own look-ahead of the
    obstacle states; the selection by the numpy rule.  Returns dict(P, X0, U0, X, U, u0, cost, status, iters, sqp_iters (per candidate), winner,
    best_cost, best_u0, gap, iterates)"""
    Kk = X.shape[0]
    P = orc.predict_params(cfg, obst)
    rs = [sequence(orc, cfg, x0, P, goal, X[k], U[k], max_iter) for k in range(Kk)]
    out = dict(P=P, X0=X.copy(), U0=U.copy(), X=np.stack([r["X"] for r in rs]), U=np.stack([r["U"] for r in rs]), u0=np.stack([r["u0"] for r in rs]),
               cost=np.array([r["cost"] for r in rs]), status=np.array([r["status"] for r in rs], np.int32),
               iters=np.array([r["iters"] for r in rs], np.int32), sqp_iters=np.array([r["sqp_iters"] for r in rs], np.int32),
               iterates=[r["iterates"] for r in rs])
    w, c = select(out["cost"], out["status"], margin)
    out.update(winner=w, best_cost=c, best_u0=out["u0"][w].copy() if w >= 0 else np.zeros(2), gap=gap(out["cost"], out["status"], margin))
    return out


_GROUP = {}


def oracle_group(orc, name, N, Tf, max_iter):
    """a parity scene's group solve from the guess family; computed once per (scene, N, Tf, max_iter) and not to be written to"""
    key = (name, N, float(Tf), max_iter)
    if key not in _GROUP:
        x0, goal, obst = scene(name)
        cfg = orc.config(N, NO, Tf)
        X, U = guesses(x0, goal, OFFSETS, N)
        _GROUP[key] = dict(cfg=cfg, x0=x0, goal=goal, obst=obst, **group_solve(orc, cfg, x0, obst, goal, X, U, max_iter))
    return _GROUP[key]


def oracle_step(orc, cfg, x, obst, goal, X, U, margin):
    """what one MultiStartMpc.step does, on the oracle, from the state (x, obst) and the member iterates (X, U) it starts from: the group solve and the
    selection, then plant step with the winner's u0 (u = 0 without a winner), obstacle step (no noise), every member on the winner's shifted iterate and
    members 1 .. K - 1 (all members without a winner) reseeded around the new state.  Returns (group_solve's dict, x, obst, X, U behind the step)"""
    r = group_solve(orc, cfg, x, obst, goal, X, U, 1, margin)
    dt = cfg.Tf / cfg.N
    xn = orc.dynamics(x, r["best_u0"], dt)[0]
    on = np.stack([orc.obstacle_step(cfg, o, dt) for o in obst])
    Xn, Un = guesses(xn, goal, OFFSETS, cfg.N)
    if r["winner"] >= 0:
        Xn[0], Un[0] = orc.shift(cfg, r["X"][r["winner"]], r["U"][r["winner"]])
    return r, xn, on, Xn, Un


_LOCKSTEP = {}


def oracle_loop(orc, name, margin, steps=LOCKSTEP_STEPS):
    """the lockstep scene driven by the oracle ALONE (the host test's conditions): a list of group_solve dicts, one per control step"""
    key = (name, float(margin), steps)
    if key not in _LOCKSTEP:
        x, goal, obst = scene(name)
        cfg = orc.config(LOCKSTEP_N, NO, LOCKSTEP_TF)
        X, U = guesses(x, goal, OFFSETS, cfg.N)
        recs = []
        for _ in range(steps):
            r, x, obst, X, U = oracle_step(orc, cfg, x, obst, goal, X, U, margin)
            recs.append(r)
        _LOCKSTEP[key] = recs
    return _LOCKSTEP[key]
