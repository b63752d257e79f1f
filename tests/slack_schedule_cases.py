"""Test infrastructure of the slack-schedule sweep (mpc_set_slack_schedule / _dev; test_slack_schedule_host.py, test_gpu_slack_schedule.py, DESIGN.md
section 4i): the explicit schedule every case runs with, the cases' problems in one form the oracle can be asked about, and the oracle-alone
conditions that make the GPU comparison mean something.  Imports without torch or a GPU; the oracle is passed in.  No test functions here.

Every solve kernel reads the schedule the same way: alpha_i = alpha[inst][i], weight alpha_i * (dt-scaled below the terminal stage, unscaled on it), rows
present at a stage >= 1 where the weight is positive.  What can go wrong there and what `schedule` therefore holds:
  * the instance index (every row different; the special rows make a neighbour's row a different PROBLEM, not a perturbation);
  * the terminal stage (alpha[N] > 0: rows the built-in schedule never has, their weight unscaled);
  * a hole inside the horizon (two adjacent stages and stage N - 1 without rows; stage 1 without rows on every fourth instance);
  * no rows at all, rows on the terminal stage alone, and the built-in schedule's own values passed back in."""
import itertools

import numpy as np

import feature_kernel_cases as fk
import sqp_cases as sc
from helpers import oracle_P, oracle_guess, random_batch

ZERO_ROW, TERMINAL_ROW, BUILTIN_ROW = 2, 3, 6      # the special rows (instances 0, 1 and 5 have roles of their own in the feature and SQP cases)
MOVED = 1e-4                                       # "the solve is another one": max |dX| beyond this
MIN_MOVED = 3


def schedule(N, B, seed, builtin=None):
    """(B, N + 1), every row different: log-uniform weights in [1e1, 1e6]; zero at the adjacent stages N // 3 and N // 3 + 1 and at stage N - 1 on
    every row, at stage 1 on every fourth; alpha[N] > 0; row ZERO_ROW all zero, row TERMINAL_ROW zero except at stage N, row BUILTIN_ROW = `builtin`
    (the built-in schedule's values of that instance, oracle.slack_alpha) -- NaN, which every setter refuses, until it is given."""
    assert B > BUILTIN_ROW and N >= 6
    rng = np.random.default_rng([N, B, seed])
    a = 10.0 ** rng.uniform(1.0, 6.0, (B, N + 1))
    a[:, [N // 3, N // 3 + 1, N - 1]] = 0.0
    a[::4, 1] = 0.0
    a[ZERO_ROW] = 0.0
    a[TERMINAL_ROW, :N] = 0.0
    a[BUILTIN_ROW] = np.nan if builtin is None else builtin
    return a


def without_terminal(alpha):
    a = alpha.copy(); a[:, -1] = 0.0
    return a


def terminal_scaled(alpha, factor):
    """the terminal stage's weight times `factor` (dt: what a kernel would use that scaled the terminal lane like the stages below it)"""
    a = alpha.copy(); a[:, -1] *= factor
    return a


def hole_filled(alpha):
    """the two adjacent zero stages given their outer neighbours' weights"""
    N = alpha.shape[1] - 1
    a = alpha.copy()
    a[:, N // 3] = a[:, N // 3 - 1]; a[:, N // 3 + 1] = a[:, N // 3 + 2]
    return a


def next_row(alpha):
    """instance b with the row of instance b + 1"""
    return np.roll(alpha, -1, axis=0)


# ---------------------------------------------------------------------------------------------------------------- problems
# A problem: dict(N, no, B, x0, goal, X0, U0, live (bool (B,): the instances that solve and are finite), groups: [dict(idx, cfg, P (on the group's
# obstacles), radii or None)], seed (of the schedule), alpha).  The oracle knows one config per call, so a batch whose instances differ in more
# than the schedule is asked about group by group.
LEVEL0_B = 37
LEVEL0_SHAPES = list(itertools.product((10, 20, 31, 40), (3, 5, 10, 2, 4, 7)))      # the (N, n_obst) grid of kernel_configs.configs

# the seed of a case's schedule: SEED unless the case is listed here (a seed that failed a condition of test_slack_schedule_host.py is replaced, the
# condition is not loosened)
SEED = 1
SEEDS = {
    ("around", 10, 3, 12, ("slack_scale_dt", 0)): 2, ("feature", 20, 2, 2): 2, ("feature", 20, 2, 3): 2, ("feature", 20, 3, 1): 6,
    ("feature", 20, 3, 2): 2, ("feature", 20, 5, 4): 5, ("feature", 20, 7, 3): 2, ("feature", 30, 2, 1): 44,
    ("feature", 30, 2, 3): 20, ("feature", 50, 3, 1): 5, ("feature", 50, 3, 2): 5, ("feature", 50, 5, 4): 11,
    ("sqp", "split3-5"): 2,
}


CROWD, CROWD_TIMED = 0.35, 0.2


def crowded(orc, cfg, x0, obst):
    """The obstacle states of the schedule sweep's world: every obstacle is aimed at a point near its instance's robot, x0 + c (position - x0),
    c = CROWD_TIMED for the obstacles that arrive later and CROWD for those there at once, which obstacle j reaches at the terminal stage
    (j % 3 == 0), at the hole N // 3 (j % 3 == 1) or at once (j % 3 == 2); velocities kept.
    The worlds of the earlier sweeps (random_batch) leave, in a batch of twelve with few obstacles, fewer than three instances with an obstacle row in
    use at a given stage -- there no schedule can be felt, whatever its seed (test_slack_schedule_host.py's conditions) -- so the sweep runs every
    case in its own world drawn closer in space and time.  The start positions are clipped into the arena; the look-ahead is the predictor's
    (which, with bug_compat_predict, moves x with vy)."""
    N, dt = cfg.N, cfg.Tf / cfg.N
    ob = obst.copy()
    near = np.array([CROWD if j % 3 == 2 else CROWD_TIMED for j in range(obst.shape[1])])
    target = x0[:, None, :2] + near[None, :, None] * (obst[:, :, :2] - x0[:, None, :2])
    vel = obst[:, :, [3, 3]] if cfg.bug_compat_predict else obst[:, :, 2:]
    when = np.array([(cfg.Tf, (N // 3 + 0.5) * dt, 0.0)[j % 3] for j in range(obst.shape[1])])
    lim = 0.95 * min(abs(float(v)) for v in cfg.arena)
    ob[:, :, :2] = np.clip(target - when[None, :, None] * vel, -lim, lim)
    return ob


def _finish(key, prob, orc):
    seed = SEEDS.get(key, SEED)
    b = BUILTIN_ROW
    own = orc.slack_alpha(next(g["cfg"] for g in prob["groups"] if b in g["idx"]), prob["x0"][b], prob["goal"][b])
    prob.update(key=key, seed=seed, alpha=schedule(prob["N"], prob["B"], seed, builtin=own))
    return prob


_PROBLEMS = {}


def level0_problem(orc, N, no, B=LEVEL0_B, cfg_kw=None, tag="level0"):
    """random_batch at the sweep's seed, the default config (or cfg_kw on top), the cold guess"""
    key = (tag, N, no, B) + tuple(sorted((cfg_kw or {}).items()))
    if key not in _PROBLEMS:
        x0, goal, obst = random_batch(B, no, seed=100 + N + no)
        cfg = orc.config(N, no, 0.1 * N, **(cfg_kw or {}))
        if cfg.soft_h:          # (hard rows: the random world as it is, in which some of the linearised problems are feasible)
            obst = crowded(orc, cfg, x0, obst)
        X0, U0 = oracle_guess(orc, cfg, x0)
        _PROBLEMS[key] = _finish(key, dict(N=N, no=no, B=B, x0=x0, goal=goal, obst=obst, X0=X0, U0=U0, live=np.ones(B, bool), cfg=cfg,
                                           groups=[dict(idx=np.arange(B), cfg=cfg, P=oracle_P(orc, cfg, obst), radii=None)]), orc)
    return _PROBLEMS[key]


WORLDS = ("crowded", "own")      # the schedule sweep's world, in which the schedule is felt (the host conditions), and the case's own inputs untouched


def feature_problem(orc, case, world="crowded"):
    """a row of feature_kernel_cases (levels 1 to 4): its inputs, group by group; the idle instance does not solve.  world "own": the inputs of
    feature_kernel_cases as they are; "crowded": their obstacles aimed at the robots"""
    key = ("feature" if world == "crowded" else "feature-own", case["N"], case["no"], case["level"])
    if key not in _PROBLEMS:
        inp = dict(fk.inputs(orc, case))
        if world == "crowded":
            base = orc.config(case["N"], case["no"], 0.1 * case["N"])
            inp["obst"] = crowded(orc, base, inp["x0"], inp["obst"])
            inp["P"] = oracle_P(orc, base, inp["obst"])
        groups = []
        for k in range(fk.GROUPS):
            idx, cfg, Pk, radii = fk.group_problem(orc, inp, k)
            groups.append(dict(idx=idx, cfg=cfg, P=Pk, radii=radii))
        X0, U0 = oracle_guess(orc, orc.config(case["N"], case["no"], 0.1 * case["N"]), inp["x0"])
        _PROBLEMS[key] = _finish(key, dict(N=inp["N"], no=inp["no"], B=fk.B, x0=inp["x0"], goal=inp["goal"], X0=X0, U0=U0, live=inp["ep_flags"] == 0,
                                           groups=groups, inp=inp), orc)
    return _PROBLEMS[key]


def sqp_problem(orc, c, world="crowded"):
    """a case of sqp_cases (level 5): its batch from the cold guess; the instance with a NaN in x0 is not finite.  world: as feature_problem's"""
    key = ("sqp" if world == "crowded" else "sqp-own", c["id"])
    if key not in _PROBLEMS:
        inp = dict(sc.inputs(orc, c))
        if world == "crowded":
            x0 = inp["x0"].copy(); x0[sc.NAN_INSTANCE, 1] = 0.0       # (the NaN instance's obstacles stay finite)
            inp["obst"] = crowded(orc, inp["cfg"], x0, inp["obst"])
            inp["P"] = oracle_P(orc, inp["cfg"], inp["obst"])
        live = np.ones(sc.B, bool); live[sc.NAN_INSTANCE] = False
        _PROBLEMS[key] = _finish(key, dict(N=inp["N"], no=inp["no"], B=sc.B, x0=inp["x0"], goal=inp["goal"], X0=inp["X0"], U0=inp["U0"], live=live, cfg=inp["cfg"],
                                           groups=[dict(idx=np.arange(sc.B), cfg=inp["cfg"], P=inp["P"], radii=None)], inp=inp), orc)
    return _PROBLEMS[key]


# the shapes of test_gpu_slack_schedule.py's tests around the kernel read (section 4 of DESIGN.md 4i): family -> (N, n_obst)
FAMILY_SHAPES = {"split": (20, 3), "one": (50, 3), "wide": (20, 20)}
AROUND_B = 12
PACKED_SHAPE = (10, 3)
SWITCHES = (dict(slack_scale_dt=0), dict(soft_h=0))


def around_problem(orc, family, cfg_kw=None):
    N, no = FAMILY_SHAPES[family]
    return level0_problem(orc, N, no, B=AROUND_B, cfg_kw=cfg_kw, tag="around")


PACKED_POOL = 2048      # the packed, scheduled batch is the first B of these instances, B just above the device's SIMD count; the oracle judges the first 64
PACKED_JUDGED = 64


def packed_problem(orc):
    return level0_problem(orc, *PACKED_SHAPE, B=PACKED_POOL, tag="packed")


def subproblem(prob, idx):
    """the instances idx of a one-group problem, as a problem"""
    (g,) = prob["groups"]
    idx = np.asarray(idx)
    return dict(key=prob["key"] + ("first", len(idx)), N=prob["N"], no=prob["no"], B=len(idx), x0=prob["x0"][idx], goal=prob["goal"][idx], obst=prob["obst"][idx],
                X0=prob["X0"][idx], U0=prob["U0"][idx], live=prob["live"][idx], cfg=prob["cfg"], seed=prob["seed"], alpha=prob["alpha"][idx],
                groups=[dict(idx=np.arange(len(idx)), cfg=g["cfg"], P=np.ascontiguousarray(g["P"][idx]), radii=None)])


def own_world_problems(orc):
    """the feature and SQP cases on their own inputs with the schedule on top: run on the GPU beside the crowded world's, so that the schedule is
    also proven on the inputs the other sweeps use; the host conditions on how many instances feel it do not hold there and are not asked"""
    out = {}
    for case in fk.enumerate_cases():
        p = feature_problem(orc, case, "own"); out[p["key"]] = p
    for c in sc.CASES:
        p = sqp_problem(orc, c, "own"); out[p["key"]] = p
    return out


def every_problem(orc):
    """every (key, problem) the GPU tests run against the oracle, once each"""
    out = {}
    for N, no in LEVEL0_SHAPES:
        p = level0_problem(orc, N, no); out[p["key"]] = p
    for case in fk.enumerate_cases():
        p = feature_problem(orc, case); out[p["key"]] = p
    for c in sc.CASES:
        p = sqp_problem(orc, c); out[p["key"]] = p
    for family in FAMILY_SHAPES:
        p = around_problem(orc, family); out[p["key"]] = p
    for kw in SWITCHES:
        p = level0_problem(orc, *PACKED_SHAPE, B=AROUND_B, cfg_kw=kw, tag="around"); out[p["key"]] = p
        p = around_problem(orc, "split", cfg_kw=kw); out[p["key"]] = p
    p = subproblem(packed_problem(orc), np.arange(PACKED_JUDGED)); out[p["key"]] = p
    return out


def oracle_solve(orc, prob, alpha, X=None, U=None, only=None):
    """one RTI solve of the problem's live instances with the schedule `alpha` (B, N + 1) from (X, U) (default the cold guess), group by group
    (`only`: that group alone); the rows of the other instances hold the iterate they started from and status -1"""
    X = prob["X0"] if X is None else X
    U = prob["U0"] if U is None else U
    B = prob["B"]
    out = dict(X=X.copy(), U=U.copy(), u0=np.zeros((B, 2)), cost=np.zeros(B), status=np.full(B, -1, np.int32), iters=np.zeros(B, np.int32))
    for k, g in enumerate(prob["groups"]):
        if only is not None and k != only:
            continue
        idx = g["idx"][prob["live"][g["idx"]]]
        if not len(idx):
            continue
        P = np.ascontiguousarray(g["P"][np.isin(g["idx"], idx)])
        with orc.obstacle_radii(g["radii"]):
            o = orc.rti_solve_batch(g["cfg"], prob["x0"][idx], P, prob["goal"][idx], X[idx], U[idx], alpha=alpha[idx])
        for key in out:
            out[key][idx] = o[key]
    return out


def moved(a, b, live):
    """how many live instances converged in both solves and differ by more than MOVED"""
    ok = live & (a["status"] == 0) & (b["status"] == 0)
    return int((np.abs(a["X"] - b["X"]).max(axis=(1, 2))[ok] > MOVED).sum())


def slack_scale(prob):
    """what the weights below the terminal stage are multiplied by: dt under slack_scale_dt, else 1"""
    cfg = prob["groups"][0]["cfg"]
    return cfg.Tf / cfg.N if cfg.slack_scale_dt else 1.0


def oracle_conditions(orc, prob, alpha=None):
    """the oracle alone on a problem: dict(first, second, cold_ok, warm_ok, iters_max, terminal, hole, row, scaled) -- whether every live instance
    converged from the cold guess and from the result, and how many instances move when alpha[N] is zeroed, the hole is filled, the neighbour's row
    is used, the terminal weight is scaled by dt like the weights of the stages below it"""
    alpha = prob["alpha"] if alpha is None else alpha
    live = prob["live"]
    first = oracle_solve(orc, prob, alpha)
    second = oracle_solve(orc, prob, alpha, first["X"], first["U"])
    return dict(first=first, second=second, cold_ok=bool((first["status"][live] == 0).all()), warm_ok=bool((second["status"][live] == 0).all()),
                iters_max=int(max(first["iters"][live].max(), second["iters"][live].max())),
                terminal=moved(first, oracle_solve(orc, prob, without_terminal(alpha)), live),
                hole=moved(first, oracle_solve(orc, prob, hole_filled(alpha)), live),
                row=moved(first, oracle_solve(orc, prob, next_row(alpha)), live),
                scaled=moved(first, oracle_solve(orc, prob, terminal_scaled(alpha, slack_scale(prob))), live))
