"""Test infrastructure of the guess family from geometry (mpc_set_guess_geometry, mpc_seed_guesses_geom_dev, MultiStartMpc(guess_geometry=...);
test_guess_geometry_host.py, test_gpu_guess_geometry.py): the numpy restatement of the rule as include/mpc_gpu.h words it, the scenes the GPU tests use
and the oracle-driven closed loop with the rule.  The iterate of an amplitude is multistart_cases.guess / guesses, reused.  Imports without torch or a
GPU; the oracle is passed in.  No test functions here.

DECISION GAP of a group: how far its inputs are from a point at which the rule's answer changes discontinuously -- the least of |s_j|, |1 - s_j| and
||c_j| - R_j| over the present obstacles with finite values, the al gaps between consecutive blocking obstacles, and ||a| - a_max| over the amplitudes used.
A comparison of the device against numpy at a tolerance is fair only where the gap is well above the rounding of both (the tests ask for 1e-6)."""
import numpy as np

import multistart_cases as mc

R_SAFE = 2.4                                   # the handle's default r_safe (mpc_default_config)
HAND = dict(clearance=0.1, a_max=6.0, lead=0.0)     # the parameters of the hand-computed answers


def amplitudes(x, goal, obst, offsets, clearance, a_max, lead, r=R_SAFE, active=None):
    """the rule for ONE group: x (5,), goal (2,), obst (n_obst, 4), offsets (K,), r a scalar or (n_obst,) radii, active None or bool (n_obst,).
    Returns (amplitudes (K,), info) with info = dict(blocks (n_obst,) bool, order = the blocking obstacles by (al, j), gap = the decision gap)."""
    x, goal, obst = np.asarray(x, dtype=np.float64), np.asarray(goal, dtype=np.float64), np.asarray(obst, dtype=np.float64)
    base = np.asarray(offsets, dtype=np.float64)
    no, K = obst.shape[0], base.shape[0]
    r = np.broadcast_to(np.asarray(r, dtype=np.float64), (no,))
    present = np.ones(no, bool) if active is None else np.asarray(active, bool)
    out = base.copy()
    d = goal - x[:2]
    L = np.sqrt(d[0] * d[0] + d[1] * d[1])
    if L < 1e-9:
        return out, dict(blocks=np.zeros(no, bool), order=[], gap=np.inf)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = d / L
        n = np.array([-t[1], t[0]])
        qx, qy = obst[:, 0] + lead * obst[:, 2], obst[:, 1] + lead * obst[:, 3]
        ex, ey = qx - x[0], qy - x[1]
        al, c = ex * t[0] + ey * t[1], ex * n[0] + ey * n[1]
        s, R = al / L, r + clearance
        blocks = present & (s > 0.0) & (s < 1.0) & (np.abs(c) < R)
        w = np.sin(np.pi * s)
        left, right = np.clip((c + R) / w, -a_max, a_max), np.clip((c - R) / w, -a_max, a_max)
    order = sorted(np.nonzero(blocks)[0].tolist(), key=lambda j: (al[j], j))
    gaps = [np.inf]
    for j in range(no):
        if present[j] and np.isfinite(s[j]) and np.isfinite(c[j]):
            gaps += [abs(s[j]), abs(1.0 - s[j]), abs(abs(c[j]) - R[j])]
    gaps += [al[b] - al[a] for a, b in zip(order[:-1], order[1:])]
    for k in range(1, K):
        m = (k - 1) // 2
        if m < len(order):
            j = order[m]
            raw = ((c[j] + R[j]) if k % 2 else (c[j] - R[j])) / w[j]
            out[k] = left[j] if k % 2 else right[j]
            gaps.append(abs(abs(raw) - a_max))
    return out, dict(blocks=blocks, order=order, gap=float(min(gaps)))


def group_amplitudes(x, goal, obst, offsets, geom, r=None, active=None):
    """tables of G groups: x (G, 5), goal (G, 2), obst (G, n_obst, 4), r None or (G, n_obst), active None or bool (G, n_obst).  Returns (amplitudes (G, K),
    gaps (G,), blockers (G,) = the number of blocking obstacles)"""
    G = x.shape[0]
    res = [amplitudes(x[g], goal[g], obst[g], offsets, geom["clearance"], geom["a_max"], geom["lead"], R_SAFE if r is None else r[g],
                      None if active is None else active[g]) for g in range(G)]
    return np.stack([a for a, _ in res]), np.array([i["gap"] for _, i in res]), np.array([len(i["order"]) for _, i in res])


def group_guesses(x, goal, amps, N):
    """the iterates of G groups from their amplitudes (G, K): X (G K, N + 1, 5), U (G K, N, 2)"""
    XU = [mc.guesses(x[g], goal[g], amps[g], N) for g in range(x.shape[0])]
    return np.concatenate([a for a, _ in XU]), np.concatenate([b for _, b in XU])


# ---------------------------------------------------------------------------------------------------------------- scenes
# the axis-aligned tie-and-clamp scene: the nearest obstacle first (and clamped), an exact tie to the lower index, the base fallback of the last member;
# every product in it is exact, so the tie is a tie on the device too
TIE = dict(x0=[-5.0, 0.0, 0.0, 0.0, 0.0], goal=[5.0, 0.0], obst=[[0.0, 0.5, 0.0, 0.0], [0.0, -0.5, 0.0, 0.0], [-4.5, 0.0, 0.0, 0.0]],
           offsets=(0.0, 2.5, -2.5, 5.0, -5.0, 1.0, -1.0, 7.0), want=(0.0, 6.0, -6.0, 3.0, -2.0, 2.0, -3.0, 7.0))
SCENE_A_WANT = (0.0, 2.7, -2.3, 5.0, -5.0)

B_MOVED = dict(mc.SCENES["B"], obst=[[0.0, 0.0, 0.0, 0.0], [3.0, 0.5, -0.5, 0.5], [-2.0, 3.0, 0.3, 0.0]])      # scene B with obstacle 1 moved: no al tie


def scene(name):
    s = B_MOVED if name == "Bm" else mc.SCENES[name]
    return np.array(s["x0"], dtype=np.float64), np.array(s["goal"], dtype=np.float64), np.array(s["obst"], dtype=np.float64)


# (scene, lead) of the hand-made GPU scenes, all at clearance 0.25, a_max 6 unless a test says otherwise
GPU_SCENES = [("A", 0.0), ("C", 0.0), ("C", 1.0), ("Bm", 0.0)]
GEOM = dict(clearance=0.25, a_max=6.0, lead=0.0)      # mpc_gpu.multistart.GUESS_GEOMETRY_DEFAULTS
RANDOM_SEED, RANDOM_G, RANDOM_NO, RANDOM_LEAD = 3, 64, 10, 0.5


def random_table(no=RANDOM_NO, G=RANDOM_G, seed=RANDOM_SEED):
    """G groups of `no` obstacles: positions and goals uniform in +-6, velocities in +-1; heading, speed and turn rate of the start drawn too"""
    rng = np.random.default_rng(seed)
    x = np.column_stack([rng.uniform(-6.0, 6.0, (G, 2)), rng.uniform(-3.0, 3.0, G), rng.uniform(0.0, 1.5, G), rng.uniform(-0.3, 0.3, G)])
    goal = rng.uniform(-6.0, 6.0, (G, 2))
    obst = np.concatenate([rng.uniform(-6.0, 6.0, (G, no, 2)), rng.uniform(-1.0, 1.0, (G, no, 2))], axis=2)
    return x, goal, obst


def hand_table(G, no, lead):
    """the hand-made scenes of GPU_SCENES at `lead` as a table of G groups of `no` obstacles (the scenes in turn), cut to the first `no` obstacles or padded
    with obstacles far outside the arena; group g + 1 is moved sideways a little against group g so that no two groups are the same"""
    names = [n for n, l in GPU_SCENES if l == lead]
    xs, gs, os_ = [], [], []
    for g in range(G):
        x0, goal, ob = scene(names[g % len(names)])
        shift = np.array([0.03125, -0.015625]) * (g // len(names))
        pad = np.tile([40.0, 40.0, 0.0, 0.0], (max(no - ob.shape[0], 0), 1))
        ob = np.concatenate([ob, pad])[:no].copy()
        x0 = x0.copy(); x0[:2] += shift; ob[:, :2] += shift
        xs.append(x0); gs.append(goal + shift); os_.append(ob)
    return np.stack(xs), np.stack(gs), np.stack(os_)


# ---------------------------------------------------------------------------------------------------------------- the closed loop with the rule, on the oracle
LOCKSTEP = [("C", 0.0), ("Bm", 0.0), ("Bm", 0.1)]
LOCKSTEP_IDS = [f"{s}-m{m}" for s, m in LOCKSTEP]
_LOOP = {}


def oracle_loop(orc, name, margin, geom=GEOM, steps=mc.LOCKSTEP_STEPS):
    """the lockstep scene driven by the oracle alone with the rule in place of the fixed family (multistart_cases.oracle_loop otherwise): per control step
    dict(winner, gap = the decision gap of the rule on the state and obstacles the NEXT solve sees, select_gap = the selection's relative cost gap, amps)"""
    key = (name, float(margin), steps, tuple(sorted(geom.items())))
    if key not in _LOOP:
        x, goal, obst = scene(name)
        cfg = orc.config(mc.LOCKSTEP_N, mc.NO, mc.LOCKSTEP_TF)
        amps, info = amplitudes(x, goal, obst, mc.OFFSETS, **geom)
        X, U = mc.guesses(x, goal, amps, cfg.N)
        recs = [dict(winner=None, gap=info["gap"], select_gap=np.inf, amps=amps)]      # the first seeding
        dt = cfg.Tf / cfg.N
        for _ in range(steps):
            r = mc.group_solve(orc, cfg, x, obst, goal, X, U, 1, margin)
            x = orc.dynamics(x, r["best_u0"], dt)[0]
            obst = np.stack([orc.obstacle_step(cfg, o, dt) for o in obst])
            amps, info = amplitudes(x, goal, obst, mc.OFFSETS, **geom)
            Xn, Un = mc.guesses(x, goal, amps, cfg.N)
            if r["winner"] >= 0:
                Xn[0], Un[0] = orc.shift(cfg, r["X"][r["winner"]], r["U"][r["winner"]])
            X, U = Xn, Un
            recs.append(dict(winner=r["winner"], gap=info["gap"], select_gap=r["gap"], amps=amps, status=r["status"]))
        _LOOP[key] = recs
    return _LOOP[key]
