"""Test infrastructure of the off-default net (test_off_default_host.py, test_gpu_off_default.py): every kernel family at a time step dt = Tf / N that
is not 0.1 and at world constants that are not the reference's -- an asymmetric arena, other slack-schedule constants, another safety radius, another
Levenberg-Marquardt term.  A fixed list of rows, each checked on the oracle alone by the host test (the counts stored here are what it asserts), the
batch generator that maps random_batch into an arena, and obstacles placed to meet every wall at a stated stage for any arena and step."""
import numpy as np

from helpers import random_batch

DEFAULT_ARENA = [-8.0, 8.0, -8.0, 8.0]      # mpc_default_config

OFF = dict(arena=[-6.5, 9.0, -9.5, 7.0], slack_a=3e3, slack_b=20.0, r_safe=1.3, lm=2e-3)

# the uniform instance parameters of the feature-level tests: cost weights that differ entry by entry (y order: x, y, v, omega, u_a, u_alpha) and OFF's radius
IP = dict(W=[1.5, 2.5, 1.0, 3.0, 0.2, 0.1], We=[4.0, 6.0, 3.0, 7.0], r_safe=OFF["r_safe"])


def scaled_batch(B, no, seed, arena):
    """helpers.random_batch with every position (x0, goal, obstacles) mapped affinely from [-8, 8]^2 into `arena` = [xmin, xmax, ymin, ymax]:
    x -> cx + x (xmax - xmin) / 16, the same for y.  Velocities and the heading are untouched; the default arena gives random_batch itself."""
    x0, goal, obst = random_batch(B, no, seed=seed)
    xmin, xmax, ymin, ymax = (float(a) for a in arena)
    for k, (lo, hi) in enumerate(((xmin, xmax), (ymin, ymax))):
        c, s = 0.5 * (lo + hi), (hi - lo) / 16.0
        x0[:, k] = c + x0[:, k] * s
        goal[:, k] = c + goal[:, k] * s
        obst[:, :, k] = c + obst[:, :, k] * s
    return x0, goal, obst


V1, V2, V3 = 1.9, 1.5, 1.8      # obstacle speeds of the wall cases (below the reference's V_MAX_OBST = 2)


def wall_cases(B, no, seed, arena, dt):
    """scaled_batch with obstacles placed against the walls of `arena` for the step `dt`: every distance is a multiple of speed x dt, so the stage in which
    a coordinate reflects is the same at every arena and step.  The look-ahead moves x with vy when bug_compat_predict (defect D1), the ground-truth step
    with vx; where a statement is about x, both velocities are equal or it says which motion it holds for.
      instance 0, obstacle 0:     1.5 steps from ymin, moving down at V1        -- y reflects in stage 2, inside the first block of four stages;
      instance 0, last obstacle:  (two or more obstacles) 6.5 steps from ymax, moving up at V2 -- y reflects in stage 7, a later block;
      instance 1, obstacle 0:     exactly on xmax, vx = vy = 1 outwards         -- x reflects in stage 1, the distance to the wall being zero;
      instance 2, last obstacle:  near the corner (xmin, ymin), vx = vy = -V2, half a step from xmin and 2.5 steps from ymin -- x reflects in stage 1, y in stage 3;
      instance 3, obstacle 0:     half a step from ymax and from xmin at (-V3, +V3) -- y reflects in stage 1; x reflects in stage 1 of the true motion only
                                  (the D1 look-ahead moves x with vy, away from xmin).
    Returns (x0, goal, obst, hits): hits = [dict(b, j, axis 0 | 1, stage, wall 'xmin' | 'xmax' | 'ymin' | 'ymax', motion 'both' | 'true')], the
    FIRST reflection of that coordinate.  All four walls are met (with one obstacle: by instances 0 .. 3 together)."""
    assert B >= 4
    x0, goal, obst = scaled_batch(B, no, seed, arena)
    xmin, xmax, ymin, ymax = (float(a) for a in arena)
    cx, cy = 0.5 * (xmin + xmax), 0.5 * (ymin + ymax)
    hits = []
    obst[0, 0] = [cx + 1.0, ymin + 1.5 * V1 * dt, 0.5, -V1]
    hits.append(dict(b=0, j=0, axis=1, stage=2, wall="ymin", motion="both"))
    obst[1, 0] = [xmax, cy + 2.0, 1.0, 1.0]
    hits.append(dict(b=1, j=0, axis=0, stage=1, wall="xmax", motion="both"))
    obst[2, no - 1] = [xmin + 0.5 * V2 * dt, ymin + 2.5 * V2 * dt, -V2, -V2]
    hits.append(dict(b=2, j=no - 1, axis=0, stage=1, wall="xmin", motion="both"))
    hits.append(dict(b=2, j=no - 1, axis=1, stage=3, wall="ymin", motion="both"))
    obst[3, 0] = [xmin + 0.5 * V3 * dt, ymax - 0.5 * V3 * dt, -V3, V3]
    hits.append(dict(b=3, j=0, axis=1, stage=1, wall="ymax", motion="both"))
    hits.append(dict(b=3, j=0, axis=0, stage=1, wall="xmin", motion="true"))
    if no >= 2:
        obst[0, no - 1] = [cx, ymax - 6.5 * V2 * dt, 0.3, V2]
        hits.append(dict(b=0, j=no - 1, axis=1, stage=7, wall="ymax", motion="both"))
    return x0, goal, obst, hits


def lookahead(arena, obst, N, dt, bug_compat=True):
    """The look-ahead of docs/PROBLEM.md section 1 ("obstacle positions") in numpy, for one obstacle state (x, y, vx, vy): constant velocity, reflection
    at the arena walls, and vx = vy when bug_compat (defect D1).  Per coordinate and stage: the time to the wall ahead is distance / |v|; if it is
    within the step, the coordinate moves to the wall and back for the rest of the step and the velocity changes sign, else it moves by v dt.
    Returns (traj (N + 1, 2), first (2,): the stage of the first reflection of x and of y, 0 for none)."""
    p = [float(obst[0]), float(obst[1])]
    v = [float(obst[3] if bug_compat else obst[2]), float(obst[3])]
    walls = ((float(arena[0]), float(arena[1])), (float(arena[2]), float(arena[3])))
    traj, first = np.zeros((N + 1, 2)), [0, 0]
    traj[0] = p
    for i in range(1, N + 1):
        for k, (lo, hi) in enumerate(walls):
            t = (p[k] - lo) / abs(v[k]) if v[k] < 0 else (hi - p[k]) / abs(v[k]) if v[k] > 0 else np.inf
            if t <= dt:
                p[k] = p[k] + (v[k] * t - v[k] * (dt - t))
                v[k] = -v[k]
                first[k] = first[k] or i
            else:
                p[k] = p[k] + v[k] * dt
        traj[i] = p
    return traj, first


# ---------------------------------------------------------------------------------------------------------------- the rows
# id: N, n_obst, B, seed of scaled_batch, Tf, how the GPU test reaches the kernel (lanes per stage, lanes per instance, wavefronts per SIMD; 0 = the
# dispatcher's choice), what kernel_name(B) starts with, and the oracle-alone counts: instances with status 0 on three consecutive solves (a cold start, two
# from the oracle's own shifted iterate) at the default constants and with OFF; `capped`: an instance of the OFF run reaches the iteration cap.
# test_off_default_host.py asserts the counts, so they are not kept by hand.
def _row(id, N, no, B, seed, Tf, lps, lpi, waves, name, ok_default, ok_off, capped=False):
    return dict(id=id, N=N, no=no, B=B, seed=seed, Tf=Tf, lps=lps, lpi=lpi, waves=waves, name=name, ok_default=ok_default, ok_off=ok_off, capped=capped)


ROWS = [
    _row("split3", 20, 3, 16, 31, 3.0, 0, 0, 0, "rti_split_kernel<3, 3", (16, 16, 16), (16, 16, 16)),
    _row("split3-w2", 20, 5, 16, 32, 3.2, 3, 0, 2, "rti_split_kernel<5, 3", (16, 16, 16), (16, 16, 16)),
    _row("split3-10", 20, 10, 16, 39, 1.4, 0, 0, 0, "rti_split_kernel<10, 3", (16, 16, 16), (16, 16, 15), capped=True),
    _row("split2", 30, 10, 16, 36, 2.1, 0, 0, 0, "rti_split_kernel<10, 2", (16, 16, 16), (16, 16, 16)),
    _row("compact-3", 62, 3, 8, 38, 9.3, 0, 0, 0, "rti_solve_kernel<3, 64, 3", (8, 8, 8), (8, 8, 8)),
    _row("compact-10", 50, 10, 16, 35, 3.5, 0, 0, 0, "rti_solve_kernel<10, 64, 3", (16, 16, 16), (15, 15, 15)),
    _row("g21", 20, 3, 16, 31, 3.0, 1, 21, 0, "rti_solve_kernel<3, 21", (16, 16, 16), (16, 16, 16)),
    _row("g32", 20, 3, 16, 31, 1.0, 1, 32, 0, "rti_solve_kernel<3, 32", (16, 16, 16), (16, 16, 15), capped=True),
    # one obstacle is fewer than the smallest row capacity (3): the dispatcher gives such a handle the stage split with partial rows whatever lane mapping is
    # asked for, so four instances per wavefront (G = 16) are reached with three obstacles at the same horizon, step, batch and seed
    _row("split3-1", 2, 1, 8, 5, 0.5, 1, 16, 0, "rti_split_kernel<3, 3, false, true", (8, 8, 8), (8, 8, 8)),
    _row("g16", 2, 3, 8, 5, 0.5, 1, 16, 0, "rti_solve_kernel<3, 16", (8, 8, 8), (8, 8, 8)),
    _row("wide20", 20, 15, 16, 34, 3.0, 0, 0, 0, "rti_wide_kernel<20", (16, 16, 16), (15, 15, 15)),
    _row("wide32", 31, 32, 8, 37, 2.48, 0, 0, 0, "rti_wide_kernel<32", (8, 8, 8), (8, 8, 8)),
    # two horizons / obstacle counts between the table's: the stage split on two lanes with a masked row capacity of 5, the compact blocks with one of 10
    _row("split2-4", 21, 4, 12, 40, 1.05, 0, 0, 0, "rti_split_kernel<5, 2", (12, 12, 12), (12, 12, 12)),
    _row("compact-7", 40, 7, 8, 41, 6.0, 0, 0, 0, "rti_solve_kernel<10, 64, 3", (8, 8, 8), (8, 8, 8)),
]
ROW = {r["id"]: r for r in ROWS}

# the acados switches away from N 20 / 3 obstacles: one cold solve per (row, switch) at the row's own Tf and the default constants; the oracle-alone counts
# of status 0 in SWITCH_OK[row][switch] (asserted by the host test).  A pair on which the oracle alone converges on fewer than B - 2 instances is dropped:
# SWITCH_DROPPED names them.
SWITCH_ROWS = ("split2", "compact-10", "g21", "wide20")
SWITCHES = ("cost_scale_dt", "slack_scale_dt", "lm_scaled", "bx_terminal", "soft_h", "bug_compat_predict")
SWITCH_VALUE = dict(cost_scale_dt=0, slack_scale_dt=0, lm_scaled=0, bx_terminal=1, soft_h=0, bug_compat_predict=0)
SWITCH_OK = {
    "split2": dict(cost_scale_dt=16, slack_scale_dt=16, lm_scaled=16, bx_terminal=16, soft_h=4, bug_compat_predict=16),
    "compact-10": dict(cost_scale_dt=16, slack_scale_dt=16, lm_scaled=16, bx_terminal=16, soft_h=1, bug_compat_predict=16),
    "g21": dict(cost_scale_dt=16, slack_scale_dt=16, lm_scaled=16, bx_terminal=16, soft_h=14, bug_compat_predict=16),
    "wide20": dict(cost_scale_dt=16, slack_scale_dt=16, lm_scaled=16, bx_terminal=16, soft_h=4, bug_compat_predict=16),
}
# hard obstacle rows make most of these random QPs with 10 and 15 obstacles infeasible (status 4 on the oracle alone: 12, 15 and 12 of 16)
SWITCH_DROPPED = (("split2", "soft_h"), ("compact-10", "soft_h"), ("wide20", "soft_h"))

# the feature-level tests (uniform instance parameters IP on OFF's arena, slack constants and LM term): rows and oracle-alone counts as above
FEATURE_OK = {"split3": (16, 16, 16), "compact-10": (15, 15, 15)}


def switch_cases():
    return [(r, sw) for r in SWITCH_ROWS for sw in SWITCHES if (r, sw) not in SWITCH_DROPPED]


def row_cfg(off):
    """config overrides of a run (mpc_gpu.BatchedMpc(**...), oracle.config(**...)): OFF or the defaults"""
    return dict(OFF) if off else {}


def configure(s, row, B=None):
    """the row's lane mapping on a fresh handle; asserts the kernel a batch of B (default: the row's) then runs"""
    if row["lps"]:
        s.set_lanes_per_stage(row["lps"])
    if row["lpi"]:
        s.set_lanes_per_instance(row["lpi"])
    if row["waves"]:
        s.set_waves_per_simd(row["waves"])
    name = s.kernel_name(row["B"] if B is None else B)
    assert name.startswith(row["name"]), (row["id"], name)
    return name


def oracle_three_solves(orc, cfg, x0, P, goal):
    """the oracle alone: a cold start, then two solves from its own shifted iterate.  Returns [(X0, U0, result)] per solve."""
    B = x0.shape[0]
    X, U = zip(*[orc.initial_guess(cfg, x) for x in x0])
    X, U = np.stack(X), np.stack(U)
    out = []
    for _ in range(3):
        o = orc.rti_solve_batch(cfg, x0, P, goal, X, U)
        out.append((X, U, o))
        X, U = o["X"].copy(), o["U"].copy()
        for b in range(B):
            X[b], U[b] = orc.shift(cfg, X[b], U[b])
    return out
