"""Test infrastructure of the group control step and its episode driver (mpc_group_step_dev, MultiStartMpc.step_fused, run_multistart_episodes;
test_multistart_episodes_host.py, test_gpu_multistart_episodes.py): the six points of include/mpc_gpu.h restated in numpy for ONE group (`tail`), over the
selection rule and the guess family of multistart_cases and the oracle's plant, obstacle step and shift; the scenes of the lockstep shapes and of the driver
test; and the oracle-side closed loop over them (`oracle_loop`), which the host test holds to the conditions the GPU tests rely on.  Imports without torch or
a GPU; the oracle is passed in.  No test functions here."""
import numpy as np

import multistart_cases as mc

TOL_GOAL = 0.15          # TOL, src/models/world_specification.py:45
R_HIT = 1.0 + 0.2        # o.r + R_ROBOT, robot_ocp_problem.py:224
MIN_NEAR = 1e-6          # no bookkeeping threshold may lie this close to the value tested against it

# the lockstep shapes (N, n_obst, K, G) and the incumbent margin each runs with; Tf = 0.1 N
SHAPES = [(2, 1, 1, 1), (20, 3, 5, 5), (62, 10, 2, 3), (31, 12, 3, 2)]
SHAPE_IDS = ["N%d-no%d-K%d-G%d" % s for s in SHAPES]
SHAPE_MARGIN = {(2, 1, 1, 1): 0.0, (20, 3, 5, 5): 0.1, (62, 10, 2, 3): 0.0, (31, 12, 3, 2): 0.0}
OFFSETS = {1: (0.0,), 2: (2.5, -2.5), 3: (0.0, 2.5, -2.5), 5: mc.OFFSETS}
STEPS = 6


def new_book():
    return dict(min_margin=np.inf, flags=0, steps=0, lost=0, switched=0)


# ---------------------------------------------------------------------------------------------------------------- the six points, one group
def tail(orc, cfg, offsets, margin, key, status, u0, x, obst, goal, X, U, noise, book, r_hit=None, active=None, margin_all=False, randomness=0.1, vmax=2.0):
    """One group's control step behind its solve.  key, status (K,), u0 (K, 2): what the solve (and the merit) left; x (5,), obst (n_obst, 4), goal (2,),
    X (K, N + 1, 5), U (K, N, 2): the group's words; noise (n_obst, 2) or None; book: new_book()'s dict; r_hit (n_obst,) and active (n_obst,) bool: row g K
    of the per-instance tables, or None.  Returns dict(idle, winner, best_key, best_u0, x, obst, X, U, book, member_x, member_obst, member_goal,
    member_flags, near) -- new arrays, the inputs are not written; `near`: the least distance of a tested value from its threshold."""
    K, N, no = len(key), cfg.N, obst.shape[0]
    x, obst, goal, X, U = (np.array(a, dtype=np.float64) for a in (x, obst, goal, X, U))
    if book["flags"] & 1:                                         # idle: every word is what it was, nothing else is defined
        return dict(idle=True, x=x, obst=obst, X=X, U=U, book=dict(book))
    dt = cfg.Tf / cfg.N
    # 1. select
    w, best = mc.select(key, status, margin)
    bu = np.array(u0[w], dtype=np.float64) if w >= 0 else np.zeros(2)
    # 2. plant, 3. obstacles
    xn = orc.dynamics(x, bu, dt)[0]
    on = np.stack([orc.obstacle_step(cfg, obst[j], dt, None if noise is None else noise[j], randomness, vmax) for j in range(no)])
    # 4. bookkeeping
    rh = np.full(no, R_HIT) if r_hit is None else np.asarray(r_hit, dtype=np.float64)
    d = np.sqrt((xn[0] - on[:, 0]) ** 2 + (xn[1] - on[:, 1]) ** 2) - rh
    counted = np.ones(no, bool) if (active is None or margin_all) else np.asarray(active, bool)
    m = d[counted].min() if counted.any() else np.inf
    b = dict(book)
    b["min_margin"] = min(book["min_margin"], m)
    ar = [cfg.arena[k] for k in range(4)]
    if xn[0] < ar[0] or xn[0] > ar[1] or xn[1] < ar[2] or xn[1] > ar[3]:
        b["flags"] |= 2
    if b["min_margin"] <= 0.0:
        b["flags"] |= 4
    dist = np.sqrt((xn[0] - goal[0]) ** 2 + (xn[1] - goal[1]) ** 2)
    if dist <= TOL_GOAL:
        b["flags"] |= 1
    else:
        b["steps"] += 1
    b["lost"] += int(w < 0)
    b["switched"] += int(w > 0)
    near = min(abs(dist - TOL_GOAL), abs(b["min_margin"]), abs(xn[0] - ar[0]), abs(xn[0] - ar[1]), abs(xn[1] - ar[2]), abs(xn[1] - ar[3]))
    # 5. next iterates
    Xn, Un = mc.guesses(xn, goal, offsets, N)
    if w >= 0:
        Xn[0], Un[0] = orc.shift(cfg, X[w], U[w])
    # 6. member inputs
    return dict(idle=False, winner=w, best_key=best, best_u0=bu, x=xn, obst=on, X=Xn, U=Un, book=b, member_x=np.tile(xn, (K, 1)), member_obst=np.tile(on, (K, 1, 1)),
                member_goal=np.tile(goal, (K, 1)), member_flags=np.full(K, b["flags"] & 1, np.int32), near=float(near))


# ---------------------------------------------------------------------------------------------------------------- scenes
def scenes(N, no, K, G, seed=0):
    """G scenes of multistart_cases (an obstacle on the line from robot to goal comes first), cut or padded to `no` obstacles -- the extra ones on a ring near
    the walls, moving --, and the explicit noise of STEPS control steps: x0 (G, 5), goal (G, 2), obst (G, no, 4), noise (STEPS, G, no, 2)"""
    names = "CBACB"
    x0, goal, obst = np.zeros((G, 5)), np.zeros((G, 2)), np.zeros((G, no, 4))
    for g in range(G):
        x, gl, ob = mc.scene(names[g % len(names)])
        x[1] += 0.05 * (g // 3)
        rows = [ob[j] for j in range(min(no, 3))]
        for j in range(3, no):
            a = 0.7 * j + 0.3 * g
            rows.append(np.array([6.3 * np.cos(a), 6.3 * np.sin(a), 0.8 * np.cos(2.0 * a), 0.8 * np.sin(2.0 * a)]))
        x0[g], goal[g], obst[g] = x, gl, np.stack(rows)
    noise = np.random.default_rng(1000 * N + 10 * no + K + seed).standard_normal((STEPS, G, no, 2))
    return x0, goal, obst, noise


def oracle_group_loop(orc, cfg, offsets, margin, x, obst, goal, noise, steps):
    """ONE group driven by the oracle alone: group solve (multistart_cases.group_solve) and `tail`, `steps` times or until the goal is reached.  Returns a
    list of dict(gap, near, winner, status, book) per control step run."""
    X, U = mc.guesses(x, goal, offsets, cfg.N)
    book, recs = new_book(), []
    for k in range(steps):
        if book["flags"] & 1:
            break
        r = mc.group_solve(orc, cfg, x, obst, goal, X, U, 1, margin)
        t = tail(orc, cfg, offsets, margin, r["cost"], r["status"], r["u0"], x, obst, goal, r["X"], r["U"], None if noise is None else noise[k], book)
        x, obst, X, U, book = t["x"], t["obst"], t["X"], t["U"], t["book"]
        recs.append(dict(gap=r["gap"], near=t["near"], winner=t["winner"], status=r["status"], book=dict(book)))
    return recs


_LOOPS = {}


def oracle_loop(orc, shape):
    """the lockstep scenes of one shape on the oracle alone: per group the records of oracle_group_loop; computed once and not to be written to"""
    if shape not in _LOOPS:
        N, no, K, G = shape
        cfg = orc.config(N, no, 0.1 * N)
        x0, goal, obst, noise = scenes(N, no, K, G)
        _LOOPS[shape] = [oracle_group_loop(orc, cfg, OFFSETS[K], SHAPE_MARGIN[shape], x0[g], obst[g], goal[g], noise[:, g], STEPS) for g in range(G)]
    return _LOOPS[shape]


# ---------------------------------------------------------------------------------------------------------------- the driver test's episodes
DRIVER = dict(G=4, K=3, N=20, Tf=2.0, no=5, max_iter=10, first_seed=0, margin=0.0)
START, GOAL = np.array([-7.0, -7.0, np.pi / 4, 0.0, 0.0]), np.array([7.0, 7.0])      # experiments.py's start and goal


def driver_inputs(world):
    """the driver test's episodes: the reference's RANDOM scenario for seeds first_seed .. first_seed + G - 1 (mpc_gpu.world, pure numpy) and explicit noise"""
    d = DRIVER
    obst = np.stack([scenario_states(world, d["first_seed"] + s, d["no"]) for s in range(d["G"])])
    noise = np.random.default_rng(77).standard_normal((d["max_iter"], d["G"], d["no"], 2))
    return np.tile(START, (d["G"], 1)), np.tile(GOAL, (d["G"], 1)), obst, noise


def scenario_states(world, seed, no):
    np.random.seed(seed)
    return np.asarray(world.obstacle_states(world.generate_random_moving_obstacles("RANDOM", n_obst=no)), dtype=np.float64).reshape(no, 4)


_DRIVER_LOOP = {}


def oracle_driver_loop(orc, world):
    if "r" not in _DRIVER_LOOP:
        d = DRIVER
        cfg = orc.config(d["N"], d["no"], d["Tf"])
        x0, goal, obst, noise = driver_inputs(world)
        _DRIVER_LOOP["r"] = [oracle_group_loop(orc, cfg, OFFSETS[d["K"]], d["margin"], x0[g], obst[g], goal[g], noise[:, g], d["max_iter"]) for g in range(d["G"])]
    return _DRIVER_LOOP["r"]
