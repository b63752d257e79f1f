"""Test infrastructure of the refill for multi-start groups and its sweep driver (mpc_group_refill_dev, run_multistart_sweep;
test_multistart_sweep_host.py, test_gpu_multistart_sweep.py): the rule of include/mpc_gpu.h restated in numpy -- `decide` (which group is kept, drained or
starts which seed index) and `apply` (keep, park, drain, start) -- over the guess family of multistart_cases, mpc_gpu.world's scenario draw under
np.random.seed and, for the seed-to-slot order of a whole sweep, episodes.refill_schedule fed with the groups' episode lengths (`simulate`); the sweep scene
of the driver tests and its closed loop on the oracle alone (`oracle_sweep`).  Imports without torch or a GPU; the oracle is passed in.  No test functions
here."""
import numpy as np

import multistart_cases as mc
import multistart_episode_cases as ec

KEEP, DRAIN = -2, -1                 # kRefillKeep, kRefillDrain (csrc/aux_kernels.hpp)
STATE_WORDS = 628                    # mt[624] | pos | has_gauss | gauss (2 words): mpc_noise_state_words()
SCENARIOS = ("RANDOM", "CENTER", "EDGE")

# the arrays of struct mpc_group_refill_arrays, in its order: name -> (rows: "G" groups, "B" members, "C" seeds, or a number; the trailing dimensions with
# -1 = n_obst, -2 = N + 1, -3 = N, -4 = STATE_WORDS; dtype)
ARRAYS = dict(x=("G", (5,), "f8"), obst=("G", (-1, 4), "f8"), goal=("G", (2,), "f8"), X=("B", (-2, 5), "f8"), U=("B", (-3, 2), "f8"), min_margin=("G", (), "f8"),
              ep_flags=("G", (), "i4"), ep_steps=("G", (), "i4"), lost=("G", (), "i4"), switched=("G", (), "i4"), state=("G", (-4,), "u4"),
              slot_seed=("G", (), "i4"), cursor=(2, (), "i4"), res_f=("C", (6,), "f8"), res_i=("C", (4,), "i4"), member_x=("B", (5,), "f8"),
              member_obst=("B", (-1, 4), "f8"), member_goal=("B", (2,), "f8"), member_flags=("B", (), "i4"))


def shape_of(name, G, K, count, N, no):
    rows, tail, _ = ARRAYS[name]
    dims = {-1: no, -2: N + 1, -3: N, -4: STATE_WORDS}
    return ({"G": G, "B": G * K, "C": max(count, 1)}.get(rows, rows),) + tuple(dims.get(d, d) for d in tail)


def first_call(G, K, count, N, no):
    """every array as the first call of a sweep wants it: slot_seed = -1, ep_flags = 1, member_flags = 1, cursor = {0, 0}; result rows not parked"""
    a = {n: np.zeros(shape_of(n, G, K, count, N, no), dtype=ARRAYS[n][2]) for n in ARRAYS}
    a["slot_seed"][:] = -1; a["ep_flags"][:] = 1; a["member_flags"][:] = 1; a["min_margin"][:] = np.inf
    a["res_f"][:] = np.nan; a["res_i"][:] = -1
    return a


# ---------------------------------------------------------------------------------------------------------------- the scenario draw
def scenario_draw(world, seed, no, scenario="RANDOM"):
    """np.random.seed(seed) and the scenario generator's draws (obstacle_generator.py:8-28 as mpc_gpu.world restates it): the obstacle states (no, 4) and
    the generator behind them in the device's layout (STATE_WORDS,) uint32 -- what mpc_generate_scenarios_dev and mpc_noise_init_dev produce for that seed"""
    np.random.seed(int(seed))
    obst = np.asarray(world.obstacle_states(world.generate_random_moving_obstacles(scenario, n_obst=no)), dtype=np.float64).reshape(no, 4)
    _, key, pos, has_gauss, cached = np.random.get_state()
    st = np.zeros(STATE_WORDS, dtype=np.uint32)
    st[:624] = key; st[624] = pos; st[625] = has_gauss
    st[626:628] = np.array([cached], dtype=np.float64).view(np.uint32)          # low word first
    return obst, st


# ---------------------------------------------------------------------------------------------------------------- the rule
def decide(ep_flags, ep_steps, handed, seed_count, max_steps):
    """the deciding launch: assign (G,) = KEEP, DRAIN or the seed index that starts, and the new cursor (handed out so far, groups that run)"""
    fin = ((np.asarray(ep_flags) & 1) != 0) | (np.asarray(ep_steps) >= max_steps)
    assign = np.full(fin.size, KEEP, dtype=np.int64)
    k = int(handed)
    for g in np.nonzero(fin)[0]:                                  # ascending group order, lowest remaining index first
        assign[g] = k if k < seed_count else DRAIN
        k += 1
    live = int((~fin).sum() + (assign >= 0).sum())
    return assign, np.array([min(k, seed_count), live], dtype=np.int32)


def apply(world, a, assign, K, N, offsets, scenario, seed_first, start, goal_rows, per_seed):
    """the applying launch on the arrays `a` (first_call's dict); returns new arrays, `a` is not written"""
    b = {n: v.copy() for n, v in a.items()}
    no = a["obst"].shape[1]
    for g, s in enumerate(assign):
        if s == KEEP:
            continue
        old = int(a["slot_seed"][g])
        if old >= 0:                                              # park
            b["res_f"][old, 0] = a["min_margin"][g]; b["res_f"][old, 1:] = a["x"][g]
            b["res_i"][old] = [a["ep_flags"][g], a["ep_steps"][g], a["lost"][g], a["switched"][g]]
        rows = slice(g * K, (g + 1) * K)
        if s == DRAIN:
            b["slot_seed"][g] = -1; b["ep_flags"][g] = a["ep_flags"][g] | 1; b["member_flags"][rows] = 1
            continue
        row = int(s) if per_seed else 0                           # start seed index s
        b["obst"][g], b["state"][g] = scenario_draw(world, seed_first + int(s), no, scenario)
        b["x"][g] = start[row]; b["goal"][g] = goal_rows[row]
        b["min_margin"][g] = np.inf
        for n in ("ep_flags", "ep_steps", "lost", "switched"):
            b[n][g] = 0
        b["slot_seed"][g] = s
        b["X"][rows], b["U"][rows] = mc.guesses(start[row], goal_rows[row], offsets, N)
        b["member_x"][rows] = b["x"][g]; b["member_obst"][rows] = b["obst"][g]; b["member_goal"][rows] = b["goal"][g]
        b["member_flags"][rows] = 0
    return b


def refill(world, a, K, N, offsets, scenario, seed_first, seed_count, max_steps, start, goal_rows, per_seed):
    """one call of mpc_group_refill_dev on the arrays `a`: (the new arrays, assign)"""
    assign, cursor = decide(a["ep_flags"], a["ep_steps"], a["cursor"][0], seed_count, max_steps)
    b = apply(world, a, assign, K, N, offsets, scenario, seed_first, np.atleast_2d(start), np.atleast_2d(goal_rows), per_seed)
    b["cursor"] = cursor
    return b, assign


def simulate(world, lengths, reached, G, K=1, N=2, no=1, max_steps=10 ** 6):
    """a whole sweep on the restatement with made-up episodes: seed index k runs lengths[k] control steps and ends on its goal where reached[k], on the
    budget otherwise (then lengths[k] must be max_steps).  Returns dict(slot, start (count,): where and at which control step each seed started; steps: the
    control steps until the sweep has drained; arrays: the final arrays)."""
    count = len(lengths)
    a = first_call(G, K, count, N, no)
    slot, begin = np.full(count, -1, dtype=np.int64), np.full(count, -1, dtype=np.int64)
    t = 0
    while True:
        a, assign = refill(world, a, K, N, (0.0,) * K, "RANDOM", 0, count, max_steps, np.zeros(5), np.ones(2), False)
        for g in np.nonzero(assign >= 0)[0]:
            slot[assign[g]], begin[assign[g]] = g, t
        if a["cursor"][1] == 0:
            return dict(slot=slot, start=begin, steps=t, arrays=a)
        for g in range(G):                                        # one control step of every group that runs
            k = int(a["slot_seed"][g])
            if a["ep_flags"][g] & 1:
                continue
            ran = a["ep_steps"][g] + 1
            if reached[k] and ran == lengths[k]:
                a["ep_flags"][g] |= 1                             # the step that reaches the goal is not counted
            else:
                a["ep_steps"][g] = ran
        t += 1


# ---------------------------------------------------------------------------------------------------------------- the sweep scene
# the reference's problem at a budget of 25 control steps; the seeds start at different distances from the goal, so that some reach it within the budget and
# at different control steps, and the others end on the budget
SWEEP = dict(N=20, Tf=2.0, no=5, K=3, count=9, first_seed=40, max_iter=25, margin=0.0, scenario="RANDOM")
GOAL = np.array([7.0, 7.0])
_AWAY = np.array([0.4, 13.0, 0.9, 3.0, 6.0, 1.2, 5.0, 0.6, 8.0])          # metres from the goal, along the diagonal the reference's start lies on
START = np.column_stack([GOAL[0] - _AWAY / np.sqrt(2.0), GOAL[1] - _AWAY / np.sqrt(2.0), np.full(9, np.pi / 4), np.zeros(9), np.zeros(9)])

_SWEEP_LOOP = {}


def oracle_sweep(orc, world):
    """the sweep scene on the oracle alone, seed by seed with the reference's noise stream: per seed the records of multistart_episode_cases.oracle_group_loop;
    computed once and not to be written to"""
    if "r" not in _SWEEP_LOOP:
        d = SWEEP
        cfg = orc.config(d["N"], d["no"], d["Tf"])
        obst, noise = world.reference_streams(d["scenario"], range(d["first_seed"], d["first_seed"] + d["count"]), n_obst=d["no"], steps=d["max_iter"])
        _SWEEP_LOOP["r"] = [ec.oracle_group_loop(orc, cfg, ec.OFFSETS[d["K"]], d["margin"], START[k], obst[k], GOAL, noise[:, k], d["max_iter"])
                            for k in range(d["count"])]
    return _SWEEP_LOOP["r"]


def lengths_of(recs):
    """(control steps run, goal reached) per seed from oracle_sweep's records"""
    return np.array([len(r) for r in recs]), np.array([bool(r[-1]["book"]["flags"] & 1) for r in recs])
