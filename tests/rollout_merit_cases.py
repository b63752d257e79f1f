"""Test infrastructure of the rollout merit (mpc_rollout_merit_dev, BatchedMpc.rollout_merit_dev, MultiStartMpc(select_by="rollout");
test_rollout_merit_host.py, test_gpu_rollout_merit.py): the random parity cases, the feature cases, and the checker's side of every output --

  X^r      by chaining oracle.dynamics from x0 (`rollout`);
  merit    oracle.cost(cfg, x0, P, goal, X^r, U) (`oracle_merit`): per-instance W / We through a config of the instance's own, per-obstacle radii through
           oracle.obstacle_radii, an obstacle mask by building the problem for the present obstacles alone;
  defect, margin, boxviol   numpy on top of oracle.dynamics, as include/mpc_gpu.h words them.

Where the oracle has no switch -- an explicit slack schedule, a per-stage reference -- `merit_np` restates the objective in numpy (the expressions of
instance_params_qp.cost and reference_qp.ls_cost, with the schedule and the mask as arguments); the host test pins it to oracle.cost on the default-feature
cases at 1e-12 relative.  Imports without torch or a GPU; the oracle is passed in.  No test functions here.

Tolerances (PROBLEM.md section 5 and a rounding bound, not the code under test): X^r, defect, margin and boxviol 1e-10 absolute -- sums of <= 62 terms of
magnitude <= 10 in another order differ by ~1e-13; three orders of room --, merit the project's cost tolerance, 1e-8 relative."""
import numpy as np

import multistart_cases as mc
from reference_qp import stage_rows

TOL_ABS = 1e-10
TOL_MERIT = 1e-8
R_HIT = 1.0 + 0.2      # the fused step's hit radius (o.r + R_ROBOT)

# the parity shapes: (N, n_obst, batch, members).  N: the smallest horizon, the default, a scan that crosses lane 32, all 63 stage lanes live; 32 obstacles at
# N = 31 (mpc_create2's handles); batch 5 leaves a partly filled workgroup; batch 9 with members 3 shares a row of x0 / P / goal among three instances
SHAPES = [(N, no, B, m) for N in (2, 20, 31, 62) for no in (1, 3, 10) for B, m in ((1, 1), (5, 1), (9, 3))] + [(31, 32, B, m) for B, m in ((1, 1), (5, 1), (9, 3))]
SHAPE_IDS = [f"N{N}-no{no}-B{B}-m{m}" for N, no, B, m in SHAPES]
PERTURB = 1e-2         # the given iterate X is X^r plus uniform noise of this size


def tf_of(N):
    return 0.1 * N     # dt = 0.1, as feature_loop.make builds its handles


# ---------------------------------------------------------------------------------------------------------------- the checker's side
def rollout(orc, x0, U, dt):
    X = np.zeros((U.shape[0] + 1, 5))
    X[0] = x0
    for i in range(U.shape[0]):
        X[i + 1] = orc.dynamics(X[i], U[i], dt)[0]
    return X


def defect(orc, x0, X, U, dt):
    d = np.abs(X[0] - x0).max()
    for i in range(U.shape[0]):
        d = max(d, np.abs(X[i + 1] - orc.dynamics(X[i], U[i], dt)[0]).max())
    return float(d)


def margin(Xr, P, r_hit=R_HIT, present=None):
    """min over stages 1 .. N and the present obstacles of |X^r_i[0:2] - P_ij| - r_hit_j; +inf with none present"""
    no = P.shape[1]
    rh = np.broadcast_to(np.asarray(r_hit, float), (no,))
    keep = np.ones(no, bool) if present is None else np.asarray(present, bool)
    if not keep.any():
        return np.inf
    d = np.sqrt(((Xr[1:, None, :2] - P[1:]) ** 2).sum(axis=2)) - rh[None, :]
    return float(d[:, keep].min())


def boxviol(Xr, lo, hi, bx_terminal=False):
    """the largest violation (>= 0) of lo <= (x, y, v, omega) <= hi at stages 1 .. N - 1, and N under bx_terminal"""
    N = Xr.shape[0] - 1
    s = Xr[1:N + 1 if bx_terminal else N][:, [0, 1, 3, 4]]
    if s.size == 0:
        return 0.0
    return float(max(0.0, (np.asarray(lo)[None, :] - s).max(), (s - np.asarray(hi)[None, :]).max()))


def builtin_alpha(cfg, x0, goal):
    """the slack schedule of robot_ocp_problem.py:145-148 (oracle.slack_alpha restated)"""
    d = np.array([x0[0] - goal[0], x0[1] - goal[1], x0[3], x0[4]])
    a = cfg.slack_a * (np.sum(d * d) + cfg.slack_b)
    return a * (cfg.N - np.arange(cfg.N + 1)) / cfg.N


def merit_np(cfg, x0, P, goal, X, U, alpha=None, R=None, W=None, We=None, r=None, present=None):
    """the NLP objective of PROBLEM.md section 3 at (X, U) in numpy: LS cost against the reference rows R (N+1, 6) (default: the goal's) with the weights
    W (6,), We (4,) (default: cfg's), plus alpha_i ss (v + v^2 / 2), v = max(0, -h), over the present obstacles with the radii r (default: cfg.r_safe)"""
    N, no = cfg.N, cfg.n_obst
    dt = cfg.Tf / N
    cs = dt if cfg.cost_scale_dt else 1.0
    wg = cs * np.array([cfg.W[k] for k in range(6)] if W is None else W, float)
    we = np.array([cfg.We[k] for k in range(4)] if We is None else We, float)
    if R is None:
        R = np.zeros((N + 1, 6)); R[:, :2] = goal
    al = builtin_alpha(cfg, x0, goal) if alpha is None else np.asarray(alpha, float)
    rr = np.broadcast_to(np.asarray(cfg.r_safe if r is None else r, float), (no,))
    keep = np.ones(no, bool) if present is None else np.asarray(present, bool)
    J = 0.0
    for i in range(N + 1):
        e = np.array([X[i, 0] - R[i, 0], X[i, 1] - R[i, 1], X[i, 3] - R[i, 2], X[i, 4] - R[i, 3]])
        if i < N:
            eu = U[i] - R[i, 4:]
            J += 0.5 * (np.sum(wg[:4] * e * e) + np.sum(wg[4:] * eu * eu))
        else:
            J += 0.5 * np.sum(we * e * e)
        z = al[i] * (dt if (cfg.slack_scale_dt and i < N) else 1.0)
        h = ((X[i, None, :2] - P[i]) ** 2).sum(axis=1) - rr ** 2
        v = np.where(h < 0, -h, 0.0)[keep]
        J += z * np.sum(v + 0.5 * v * v)
    return float(J)


def config_like(cfg, **kw):
    """a copy of an oracle config with fields replaced (arrays element by element)"""
    c = type(cfg).from_buffer_copy(cfg)
    for k, v in kw.items():
        cur = getattr(c, k)
        if hasattr(cur, "__len__"):
            for i, x in enumerate(v):
                cur[i] = x
        else:
            setattr(c, k, v)
    return c


def oracle_merit(orc, cfg, x0, P, goal, X, U, W=None, We=None, r=None, present=None):
    """oracle.cost at (X, U): W / We through a config of the instance's own, radii through oracle.obstacle_radii, a mask by building the problem for the
    present obstacles alone (at least one must be present: the oracle has no problem without obstacles)"""
    kw = {}
    if W is not None:
        kw["W"] = list(W)
    if We is not None:
        kw["We"] = list(We)
    if present is not None:
        keep = np.nonzero(np.asarray(present, bool))[0]
        assert len(keep) >= 1
        kw["n_obst"] = len(keep)
        P = np.ascontiguousarray(P[:, keep])
        r = None if r is None else np.asarray(r, float)[keep]
    c = config_like(cfg, **kw) if kw else cfg
    with orc.obstacle_radii(None if r is None else np.broadcast_to(np.asarray(r, float), (c.n_obst,)).copy()):
        return float(orc.cost(c, x0, P, goal, X, U))


# ---------------------------------------------------------------------------------------------------------------- the random parity cases
_CASES = {}


def case(orc, N, no, B, members, seed=None):
    """one random parity case, computed once and not to be written to: rows = ceil(B / members) scenario rows of x0 (rows, 5), goal (rows, 2), obst
    (rows, no, 4) and P (rows, N+1, no, 2); per instance U (B, N, 2) uniform within the input bounds, Xr (B, N+1, 5) the oracle's rollout and
    X = Xr + uniform(-PERTURB, PERTURB); and the checker's outputs merit, defect, margin, boxviol (B,), cost_X = oracle.cost at the GIVEN (X, U)"""
    key = (N, no, B, members, seed)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(1000 * N + 10 * no + B + 3 if seed is None else seed)
    cfg = orc.config(N, no, tf_of(N))
    dt = cfg.Tf / N
    rows = -(-B // members)
    x0 = np.zeros((rows, 5))
    x0[:, :2] = rng.uniform(-4, 4, (rows, 2)); x0[:, 2] = rng.uniform(-3, 3, rows); x0[:, 3] = rng.uniform(-1, 1, rows); x0[:, 4] = rng.uniform(-0.5, 0.5, rows)
    goal = rng.uniform(-6, 6, (rows, 2))
    obst = np.zeros((rows, no, 4))
    obst[:, :, :2] = rng.uniform(-6, 6, (rows, no, 2)); obst[:, :, 2:] = rng.uniform(-2, 2, (rows, no, 2))
    P = np.stack([orc.predict_params(cfg, o) for o in obst])
    U = rng.uniform([cfg.bu_lo[0], cfg.bu_lo[1]], [cfg.bu_hi[0], cfg.bu_hi[1]], (B, N, 2))
    Xr = np.stack([rollout(orc, x0[b // members], U[b], dt) for b in range(B)])
    X = Xr + rng.uniform(-PERTURB, PERTURB, Xr.shape)
    lo, hi = [cfg.bx_lo[k] for k in range(4)], [cfg.bx_hi[k] for k in range(4)]
    out = dict(cfg=cfg, dt=dt, rows=rows, members=members, x0=x0, goal=goal, obst=obst, P=P, U=U, X=X, Xr=Xr,
               merit=np.array([oracle_merit(orc, cfg, x0[b // members], P[b // members], goal[b // members], Xr[b], U[b]) for b in range(B)]),
               cost_X=np.array([oracle_merit(orc, cfg, x0[b // members], P[b // members], goal[b // members], X[b], U[b]) for b in range(B)]),
               defect=np.array([defect(orc, x0[b // members], X[b], U[b], dt) for b in range(B)]),
               margin=np.array([margin(Xr[b], P[b // members]) for b in range(B)]),
               boxviol=np.array([boxviol(Xr[b], lo, hi, bool(cfg.bx_terminal)) for b in range(B)]))
    _CASES[key] = out
    return out


# ---------------------------------------------------------------------------------------------------------------- the feature cases
FEATURE_SHAPE = (20, 3, 5, 1)      # N, n_obst, batch, members of every feature case
FEATURES = ("alpha", "reference", "params", "mask", "bounds")
MIN_EFFECT = 1e-4                  # relative change of the figure a feature case must show against the same call without the feature


def feature(orc, name):
    """what a feature case sets on the handle (`set`: keyword arguments of the BatchedMpc setter named `setter`) and the checker's figures with it: merit,
    margin, boxviol (B,), each equal to the base case's where the feature does not reach it.  The base case is case(orc, *FEATURE_SHAPE)."""
    N, no, B, m = FEATURE_SHAPE
    c = case(orc, N, no, B, m)
    cfg, x0, goal, P, U, Xr = c["cfg"], c["x0"], c["goal"], c["P"], c["U"], c["Xr"]
    rng = np.random.default_rng(77)
    out = dict(merit=c["merit"].copy(), margin=c["margin"].copy(), boxviol=c["boxviol"].copy(), by_oracle=True)
    if name == "alpha":          # an explicit schedule with a hole: three stages without a penalty, the others at twice the built-in weight
        alpha = np.stack([2.0 * builtin_alpha(cfg, x0[b], goal[b]) for b in range(B)])
        alpha[:, 4:7] = 0.0
        out.update(setter="set_slack_schedule", set=dict(alpha=alpha), by_oracle=False,
                   merit=np.array([merit_np(cfg, x0[b], P[b], goal[b], Xr[b], U[b], alpha=alpha[b]) for b in range(B)]))
    elif name == "reference":    # a per-stage reference with a non-zero offset
        T = N + 6
        yref = rng.uniform(-3, 3, (B, T, 6))
        off = np.array([3, 0, 5, 1, 4], np.int32)
        out.update(setter="set_reference", set=dict(yref=yref, offset=off), by_oracle=False,
                   merit=np.array([merit_np(cfg, x0[b], P[b], goal[b], Xr[b], U[b], R=stage_rows(yref[b], off[b], N)) for b in range(B)]))
    elif name == "params":       # per-instance W / We / r_safe / r_hit
        W = np.array([cfg.W[k] for k in range(6)]) * np.exp(rng.uniform(np.log(0.25), np.log(4.0), (B, 6)))
        We = np.array([cfg.We[k] for k in range(4)]) * np.exp(rng.uniform(np.log(0.25), np.log(4.0), (B, 4)))
        r_safe, r_hit = rng.uniform(1.6, 3.0, (B, no)), rng.uniform(0.5, 2.0, (B, no))
        out.update(setter="set_instance_params", set=dict(W=W, We=We, r_safe=r_safe, r_hit=r_hit),
                   merit=np.array([oracle_merit(orc, cfg, x0[b], P[b], goal[b], Xr[b], U[b], W=W[b], We=We[b], r=r_safe[b]) for b in range(B)]),
                   merit_np=np.array([merit_np(cfg, x0[b], P[b], goal[b], Xr[b], U[b], W=W[b], We=We[b], r=r_safe[b]) for b in range(B)]),
                   margin=np.array([margin(Xr[b], P[b], r_hit[b]) for b in range(B)]))
    elif name == "mask":         # every instance loses the obstacle its rollout comes closest to; the last instance keeps that one alone
        closest = np.array([np.argmin([margin(Xr[b], P[b], present=np.arange(no) == j) for j in range(no)]) for b in range(B)])
        active = np.arange(no)[None, :] != closest[:, None]
        active[B - 1] = ~active[B - 1]
        out.update(setter="set_obstacle_mask", set=dict(active=active),
                   merit=np.array([oracle_merit(orc, cfg, x0[b], P[b], goal[b], Xr[b], U[b], present=active[b]) for b in range(B)]),
                   merit_np=np.array([merit_np(cfg, x0[b], P[b], goal[b], Xr[b], U[b], present=active[b]) for b in range(B)]),
                   margin=np.array([margin(Xr[b], P[b], present=active[b]) for b in range(B)]))
    elif name == "bounds":       # a small per-instance speed bound
        bx_hi = np.tile([cfg.bx_hi[k] for k in range(4)], (B, 1)); bx_lo = np.tile([cfg.bx_lo[k] for k in range(4)], (B, 1))
        bx_hi[:, 2] = rng.uniform(0.2, 0.6, B); bx_lo[:, 3] = -rng.uniform(0.1, 0.3, B)
        out.update(setter="set_instance_bounds", set=dict(bx_lo=bx_lo, bx_hi=bx_hi),
                   boxviol=np.array([boxviol(Xr[b], bx_lo[b], bx_hi[b], bool(cfg.bx_terminal)) for b in range(B)]))
    else:
        raise KeyError(name)
    return out


def rel_change(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)
    return np.where(np.isfinite(a) & np.isfinite(b), d, np.where(a == b, 0.0, np.inf))


# ---------------------------------------------------------------------------------------------------------------- multi-start by rollout merit
# the scenes of multistart_cases and one of this module's: the obstacle sits just beside the line, so that the straight member's linearised step cuts through
# it (cheap at face value, expensive on the plant)
SCENES = dict(mc.SCENES)
SCENES["D"] = dict(x0=[-5.0, 0.0, 0.0, 2.0, 0.0], goal=[5.0, 0.0], obst=[[-1.0, 0.6, 0.0, 0.0], [2.5, -1.0, 0.0, 0.3], [-2.0, 4.0, 0.3, 0.0]])
MS_SCENES = ("A", "B", "C", "D")
MS_N, MS_TF = 20, 2.0
MS_MARGIN_SCENE = ("B", 0.1)                    # the scene that is also selected with a margin
MS_LOCKSTEP = [("C", 0.0), ("D", 0.0), ("B", 0.1)]
MS_LOCKSTEP_IDS = [f"{s}-m{m}" for s, m in MS_LOCKSTEP]
MS_STEPS = 4


def ms_scene(name):
    s = SCENES[name]
    return np.array(s["x0"], dtype=np.float64), np.array(s["goal"], dtype=np.float64), np.array(s["obst"], dtype=np.float64)


def group_solve(orc, cfg, x0, obst, goal, X, U, margin_m=0.0):
    """multistart_cases.group_solve (one RTI iteration per candidate) with the checker's rollout figures per candidate -- merit, defect, margin (K,) -- and the
    selection by the numpy rule on the MERITS: winner, best_cost (the winner's merit), best_u0, gap; winner_by_cost is the rule on the reported costs"""
    r = mc.group_solve(orc, cfg, x0, obst, goal, X, U, 1, margin_m)
    dt = cfg.Tf / cfg.N
    Kk = X.shape[0]
    Xr = [rollout(orc, x0, r["U"][k], dt) for k in range(Kk)]
    r["winner_by_cost"] = r["winner"]
    r["merit"] = np.array([orc.cost(cfg, x0, r["P"], goal, Xr[k], r["U"][k]) for k in range(Kk)])
    r["defect"] = np.array([defect(orc, x0, r["X"][k], r["U"][k], dt) for k in range(Kk)])
    r["margin"] = np.array([margin(Xr[k], r["P"]) for k in range(Kk)])
    w, c = mc.select(r["merit"], r["status"], margin_m)
    r.update(winner=w, best_cost=c, best_u0=r["u0"][w].copy() if w >= 0 else np.zeros(2), gap=mc.gap(r["merit"], r["status"], margin_m))
    return r


_MS = {}


def ms_group(orc, name, margin_m=0.0):
    """a scene's group solve from the guess family, selected by merit; computed once per (scene, margin) and not to be written to"""
    key = (name, float(margin_m))
    if key not in _MS:
        x0, goal, obst = ms_scene(name)
        cfg = orc.config(MS_N, mc.NO, MS_TF)
        X, U = mc.guesses(x0, goal, mc.OFFSETS, MS_N)
        _MS[key] = dict(cfg=cfg, x0=x0, goal=goal, obst=obst, **group_solve(orc, cfg, x0, obst, goal, X, U, margin_m))
    return _MS[key]


def ms_step(orc, cfg, x, obst, goal, X, U, margin_m):
    """multistart_cases.oracle_step with the selection by merit"""
    r = group_solve(orc, cfg, x, obst, goal, X, U, margin_m)
    dt = cfg.Tf / cfg.N
    xn = orc.dynamics(x, r["best_u0"], dt)[0]
    on = np.stack([orc.obstacle_step(cfg, o, dt) for o in obst])
    Xn, Un = mc.guesses(xn, goal, mc.OFFSETS, cfg.N)
    if r["winner"] >= 0:
        Xn[0], Un[0] = orc.shift(cfg, r["X"][r["winner"]], r["U"][r["winner"]])
    return r, xn, on, Xn, Un


_MS_LOOP = {}


def ms_loop(orc, name, margin_m, steps=MS_STEPS):
    """the lockstep scene driven by the oracle alone, selected by merit: a list of group_solve dicts, one per control step"""
    key = (name, float(margin_m), steps)
    if key not in _MS_LOOP:
        x, goal, obst = ms_scene(name)
        cfg = orc.config(MS_N, mc.NO, MS_TF)
        X, U = mc.guesses(x, goal, mc.OFFSETS, cfg.N)
        recs = []
        for _ in range(steps):
            r, x, obst, X, U = ms_step(orc, cfg, x, obst, goal, X, U, margin_m)
            recs.append(r)
        _MS_LOOP[key] = recs
    return _MS_LOOP[key]
