"""The refill for multi-start groups and its sweep driver without a GPU: the numpy restatement of the rule (multistart_sweep_cases: keep, park, drain,
start) on its degenerate ends and, over made-up episodes, against episodes.refill_schedule fed with the groups' episode lengths; the agreement of header,
binding and struct mirror on mpc_group_refill_dev; the driver's refusals, which come before a handle exists; and the ORACLE-ALONE CONDITIONS
test_gpu_multistart_sweep.py relies on for the sweep scene, stated as asserts:

  1. the episode lengths take at least 3 distinct values; at least one seed ends on its budget and at least one on its goal;
  2. every selection is a relative gap >= 1e-4 (multistart_cases.MIN_GAP) from going the other way;
  3. no bookkeeping threshold (goal tolerance, arena edge, margin 0) lies within 1e-6 (multistart_episode_cases.MIN_NEAR) of the value tested against it.
A scene that fails a condition is to be replaced, not the threshold lowered.  The figures are printed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import multistart_cases as mc
import multistart_episode_cases as ec
import multistart_sweep_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mpc_group_refill_dev"


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


@pytest.fixture(scope="module")
def lib(built):
    from mpc_gpu import _lib
    return _lib


@pytest.fixture(scope="module")
def world():
    from mpc_gpu import world
    return world


@pytest.fixture(scope="module", autouse=True)
def the_restatement_is_over_the_structs_arrays():
    """the arrays the restatement keeps are the fields of mpc_group_refill_arrays, in its order: a field added to one and not the other fails every test here"""
    from mpc_gpu import _lib
    assert list(sc.ARRAYS) == [n for n, _ in _lib.GroupRefillArrays._fields_]


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpc_gpu.h")).read(), flags=re.S)


def test_header_and_binding_agree_on_the_prototype_the_struct_and_the_abi_version(lib):
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{NAME} is not declared in include/mpc_gpu.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert len(args) == 14, args
    assert [re.search(r"(\w+)$", a).group(1) for a in args] == ["h", "groups", "K", "scenario", "seed_first", "seed_count", "max_steps", "box", "d_start",
                                                               "d_goal_rows", "per_seed", "d_offsets", "a", "stream"]
    want = [C.POINTER(lib.GroupRefillArrays) if "mpc_group_refill_arrays" in a else (C.c_void_p if "*" in a else {"int": C.c_int, "unsigned": C.c_uint}[a.split()[0]])
            for a in args]
    res, bound = lib.SYMBOLS[NAME]
    assert res is C.c_int and bound == want, (args, bound)
    assert hasattr(C.CDLL(lib.LIB_PATH), NAME)
    body = re.search(r"typedef struct mpc_group_refill_arrays\s*\{(.*?)\}\s*mpc_group_refill_arrays\s*;", _header(), flags=re.S).group(1)
    fields = [f.strip().lstrip("*") for decl in body.split(";") if decl.strip() for f in decl.split("*", 1)[1].split(",")]
    assert fields == [n for n, _ in lib.GroupRefillArrays._fields_] == list(sc.ARRAYS), fields
    assert C.sizeof(lib.GroupRefillArrays) == 8 * len(fields)
    hdr = open(os.path.join(ROOT, "include", "mpc_gpu.h")).read()
    assert int(re.search(r"#define\s+MPC_ABI_VERSION\s+(\d+)", hdr).group(1)) == lib.ABI_VERSION == lib.lib().mpc_abi_version()
    assert lib.lib().mpc_noise_state_words() == sc.STATE_WORDS


def test_argument_errors_that_need_no_device(lib):
    L = lib.lib()
    arr = lib.GroupRefillArrays()
    box = (C.c_double * 6)()
    call = lambda h=None, G=1, K=3: L.mpc_group_refill_dev(h, G, K, 0, 0, 1, 1, box, None, None, 0, None, arr, None)
    assert call() == lib.MPC_ERR_ARG and b"null handle" in L.mpc_last_error()


# ---------------------------------------------------------------------------------------------------------------- the driver's refusals
def test_the_driver_refuses_bad_arguments_before_any_device_use(monkeypatch):
    import mpc_gpu
    from mpc_gpu import multistart as ms
    assert mpc_gpu.run_multistart_sweep is ms.run_multistart_sweep and "run_multistart_sweep" in mpc_gpu.__all__

    def no_handle(*a, **k):
        raise AssertionError("a handle was made before the arguments were checked")
    monkeypatch.setattr(ms, "MultiStartMpc", type("Refuse", (), {"__init__": no_handle}))
    start, goal = [-7.0, -7.0, np.pi / 4, 0.0, 0.0], [7.0, 7.0]
    ok = ms.sweep_arguments(start, goal, "RANDOM", (40, 9), 4, max_iter=25)
    assert (ok["first"], ok["count"], ok["S"], ok["K"], ok["per_seed"], ok["bound"]) == (40, 9, 4, 5, False, 3 * 25 + 25) and ok["start"].shape == (1, 5)
    ok = ms.sweep_arguments(sc.START, goal, "EDGE", range(40, 49), 20, offsets=(0.0, 1.0), poll_every=1, max_iter=25)
    assert (ok["S"], ok["K"], ok["per_seed"], ok["bound"]) == (9, 2, True, 26) and ok["goal"].shape == (9, 2)      # no more group slots than seeds
    bad = [dict(seeds=range(0, 20, 2)), dict(seeds=(0, 0)), dict(seeds=10), dict(seeds=(-1, 4)), dict(start=np.zeros((7, 5))), dict(goal=np.zeros((3, 2))),
           dict(start=np.zeros(4)), dict(slots=0), dict(slots=2.5), dict(scenario=np.zeros((9, 5, 4))), dict(scenario="CORNER"), dict(max_iter=0),
           dict(poll_every=0), dict(offsets=[]), dict(offsets=np.zeros(65)), dict(offsets=[0.0, np.nan]), dict(incumbent_margin=1.0),
           dict(incumbent_margin=-0.1), dict(incumbent_margin=float("nan")), dict(select_by="merit"), dict(n_obst=0), dict(n_obst=33), dict(sqp=3),
           dict(solver=object())]
    for kw in bad:
        args = dict(start=start, goal=goal, scenario="RANDOM", seeds=(40, 9), slots=4)
        args.update(kw)
        with pytest.raises(ValueError):
            ms.run_multistart_sweep(args.pop("start"), args.pop("goal"), args.pop("scenario"), args.pop("seeds"), args.pop("slots"), **args)
    for kw in [dict(r_safe=np.ones(9)), dict(r_hit=np.ones(9)), dict(W=np.ones((9, 6))), dict(We=np.ones((9, 4))), dict(active=np.ones((9, 5), bool)),
               dict(bounds=dict(bu_lo=[-1.0, -1.0])), dict(status_log=True), dict(ring=8), dict(trace=True), dict(trace=[0, 1]), dict(record=True),
               dict(noise="torch"), dict(first_seed=3)]:      # not offered: there is no such argument
        with pytest.raises(TypeError):
            ms.run_multistart_sweep(start, goal, "RANDOM", (40, 9), 4, **kw)


# ---------------------------------------------------------------------------------------------------------------- the restatement on its ends
N, NO, K, G = 4, 2, 3, 4
OFF = ec.OFFSETS[K]


def _running(world, count=6, first=11, per_seed=True):
    """G groups that run seeds 0 .. G - 1 after the first call, with some bookkeeping behind them"""
    start, goal = np.arange(5.0 * count).reshape(count, 5) / 10.0 - 1.0, np.arange(2.0 * count).reshape(count, 2) / 3.0 + 1.0
    if not per_seed:
        start, goal = start[:1], goal[:1]
    a, assign = sc.refill(world, sc.first_call(G, K, count, N, NO), K, N, OFF, "RANDOM", first, count, 10, start, goal, per_seed)
    rng = np.random.default_rng(5)
    a["ep_steps"][:] = [3, 4, 5, 6]; a["lost"][:] = [0, 1, 0, 2]; a["switched"][:] = [1, 0, 2, 0]; a["min_margin"][:] = [0.5, -0.1, 2.0, 0.3]
    a["x"][:] = rng.uniform(-5, 5, (G, 5)); a["X"][:] = rng.uniform(-5, 5, a["X"].shape); a["U"][:] = rng.uniform(-1, 1, a["U"].shape)
    return a, assign, start, goal


def _same(a, b, but=()):
    return all(np.array_equal(a[n], b[n], equal_nan=True) for n in a if n not in but)


def test_the_first_call_fills_every_group(world):
    a, assign, start, goal = _running(world)
    assert assign.tolist() == [0, 1, 2, 3]
    b, _ = sc.refill(world, sc.first_call(G, K, 6, N, NO), K, N, OFF, "RANDOM", 11, 6, 10, start, goal, True)
    assert b["slot_seed"].tolist() == [0, 1, 2, 3] and b["cursor"].tolist() == [4, 4] and not b["ep_flags"].any() and not b["member_flags"].any()
    assert np.isinf(b["min_margin"]).all() and np.isnan(b["res_f"]).all() and (b["res_i"] == -1).all()          # nothing to park: no group held a seed
    for g in range(G):
        obst, st = sc.scenario_draw(world, 11 + g, NO)
        assert np.array_equal(b["obst"][g], obst) and np.array_equal(b["state"][g], st) and st[624] == 8 * NO and not st[625:].any()
        assert np.array_equal(b["x"][g], start[g]) and np.array_equal(b["goal"][g], goal[g])
        Xg, Ug = mc.guesses(start[g], goal[g], OFF, N)
        rows = slice(g * K, (g + 1) * K)
        assert np.array_equal(b["X"][rows], Xg) and not b["U"][rows].any() and np.array_equal(b["X"][rows][:, 0], np.tile(start[g], (K, 1)))
        assert (b["member_x"][rows] == start[g]).all() and (b["member_obst"][rows] == obst).all() and (b["member_goal"][rows] == goal[g]).all()
    assert np.array_equal(sc.scenario_draw(world, 11, NO, "EDGE")[0][:, :2], np.full((NO, 2), 7.0)) and sc.scenario_draw(world, 11, NO, "CENTER")[1][624] == 4 * NO


def test_nothing_finished_writes_nothing_but_the_live_count(world):
    a, _, start, goal = _running(world)
    b, assign = sc.refill(world, a, K, N, OFF, "RANDOM", 11, 6, 10, start, goal, True)
    assert (assign == sc.KEEP).all() and _same(a, b) and b["cursor"].tolist() == [4, 4]


def test_a_mixed_call_keeps_parks_starts_and_drains(world):
    a, _, start, goal = _running(world, count=5)
    a["ep_flags"][1] = 5                                          # finished by its flag (and hit) -> starts seed index 4, the last one
    a["ep_steps"][3] = 10                                         # finished by the budget alone -> no seed is left: drained
    b, assign = sc.refill(world, a, K, N, OFF, "RANDOM", 11, 5, 10, start, goal, True)
    assert assign.tolist() == [sc.KEEP, 4, sc.KEEP, sc.DRAIN] and b["cursor"].tolist() == [5, 3]
    for g in (0, 2):                                              # kept: every word of the group and of its members
        rows = slice(g * K, (g + 1) * K)
        for n, (r, _, _) in sc.ARRAYS.items():
            if r in ("G", "B"):
                assert np.array_equal(a[n][rows if r == "B" else g], b[n][rows if r == "B" else g]), (n, g)
    assert b["res_f"][1].tolist() == [-0.1] + a["x"][1].tolist() and b["res_i"][1].tolist() == [5, 4, 1, 0]
    assert b["res_f"][3].tolist() == [0.3] + a["x"][3].tolist() and b["res_i"][3].tolist() == [0, 10, 2, 0]      # the budget's row has bit 0 clear
    assert np.isnan(b["res_f"][[0, 2, 4]]).all() and (b["res_i"][[0, 2, 4]] == -1).all()
    assert b["slot_seed"].tolist() == [0, 4, 2, -1] and b["ep_flags"].tolist() == [0, 0, 0, 1] and b["ep_steps"].tolist() == [3, 0, 5, 10]
    assert b["member_flags"].tolist() == [0] * 9 + [1] * 3
    for n in ("x", "obst", "goal", "X", "U", "min_margin", "lost", "switched", "state", "member_x", "member_obst", "member_goal"):      # a drain writes nothing else
        assert np.array_equal(a[n][9:12] if sc.ARRAYS[n][0] == "B" else a[n][3], b[n][9:12] if sc.ARRAYS[n][0] == "B" else b[n][3]), n
    assert np.array_equal(b["x"][1], start[4]) and np.array_equal(b["obst"][1], sc.scenario_draw(world, 15, NO)[0]) and b["lost"][1] == 0 and np.isinf(b["min_margin"][1])
    again, assign = sc.refill(world, b, K, N, OFF, "RANDOM", 11, 5, 10, start, goal, True)          # a drained group is drained again: the same words
    assert assign.tolist() == [sc.KEEP, sc.KEEP, sc.KEEP, sc.DRAIN] and _same(b, again)


def test_everything_finished_with_fewer_seeds_than_groups(world):
    a, _, start, goal = _running(world, count=6)
    a["ep_flags"][:] = [1, 3, 1, 1]
    b, assign = sc.refill(world, a, K, N, OFF, "RANDOM", 11, 6, 10, start, goal, True)
    assert assign.tolist() == [4, 5, sc.DRAIN, sc.DRAIN] and b["cursor"].tolist() == [6, 2] and b["slot_seed"].tolist() == [4, 5, -1, -1]
    assert (b["res_i"][:4, 0] == [1, 3, 1, 1]).all() and (b["res_i"][4:] == -1).all() and b["member_flags"].tolist() == [0] * 6 + [1] * 6
    c, assign = sc.refill(world, dict(b, ep_flags=np.array([1, 1, 1, 1], np.int32)), K, N, OFF, "RANDOM", 11, 6, 10, start, goal, True)
    assert (assign == sc.DRAIN).all() and c["cursor"].tolist() == [6, 0] and (c["res_i"][:, 0] >= 0).all() and (c["slot_seed"] == -1).all()


def test_one_member_and_one_row_for_all_seeds(world):
    start, goal = np.array([[-3.0, 1.0, 0.2, 1.0, 0.1]]), np.array([[5.0, 2.0]])
    b, assign = sc.refill(world, sc.first_call(2, 1, 3, N, NO), 1, N, (2.5,), "CENTER", 0, 3, 10, start, goal, False)
    assert assign.tolist() == [0, 1] and b["X"].shape == (2, N + 1, 5) and np.array_equal(b["X"][0], mc.guess(start[0], goal[0], 2.5, N)[0])
    assert np.array_equal(b["x"], np.tile(start, (2, 1))) and np.array_equal(b["member_x"], b["x"]) and not b["obst"][:, :, :2].any()
    assert not np.array_equal(b["obst"][0], b["obst"][1])          # the seeds differ, the rows do not


def test_no_seeds_at_all_drains_every_group(world):
    a = sc.first_call(3, 2, 0, N, NO)
    b, assign = sc.refill(world, a, 2, N, (0.0, 1.0), "RANDOM", 0, 0, 10, np.zeros((1, 5)), np.ones((1, 2)), False)
    assert (assign == sc.DRAIN).all() and b["cursor"].tolist() == [0, 0] and _same(a, b, but=("cursor",))


@pytest.mark.parametrize("slots", [1, 2, 4, 9, 12])
def test_a_whole_sweep_follows_refill_schedule_on_the_groups_episode_lengths(world, slots):
    from mpc_gpu.episodes import refill_schedule
    lengths = np.array([14, 25, 20, 21, 25, 23, 25, 16, 25]); reached = lengths < 25
    reached[4] = True                                             # a goal reached on the budget's last step is a goal reached
    sim = sc.simulate(world, lengths, reached, min(slots, 9), max_steps=25)
    want = refill_schedule(lengths, slots)
    assert np.array_equal(sim["slot"], want["slot"]) and np.array_equal(sim["start"], want["start"]) and sim["steps"] == want["steps"]
    ri = sim["arrays"]["res_i"]
    assert np.array_equal(ri[:, 1] + (ri[:, 0] & 1), lengths) and np.array_equal((ri[:, 0] & 1) != 0, reached)


# ---------------------------------------------------------------------------------------------------------------- the oracle-alone conditions
def test_the_sweep_scene_meets_the_conditions_on_every_step(orc, world):
    d = sc.SWEEP
    recs = sc.oracle_sweep(orc, world)
    lengths, reached = sc.lengths_of(recs)
    gaps, nears = [min(r["gap"] for r in rec) for rec in recs], [min(r["near"] for r in rec) for rec in recs]
    for k, rec in enumerate(recs):
        print(f"MULTISTART-SWEEP-HOST seed {d['first_seed'] + k} from {np.linalg.norm(sc.START[k, :2] - sc.GOAL):.2f} m: {lengths[k]} control steps, reached {bool(reached[k])}, "
              f"flags {rec[-1]['book']['flags']}, switched {rec[-1]['book']['switched']}, least gap {gaps[k]:.3e}, least distance from a threshold {nears[k]:.3e}")
    print(f"MULTISTART-SWEEP-HOST least gap seen {min(gaps):.3e}, least distance from a threshold {min(nears):.3e}, lengths {lengths.tolist()}")
    assert len(recs) == d["count"] == 9 and d["first_seed"] > 0 and len(set(np.linalg.norm(sc.START[:, :2] - sc.GOAL, axis=1).round(6))) == 9
    assert len(set(lengths.tolist())) >= 3
    budget = (lengths == d["max_iter"]) & ~reached
    assert budget.any() and reached.any() and (reached | budget).all()
    assert min(gaps) >= mc.MIN_GAP, gaps
    assert min(nears) >= ec.MIN_NEAR, nears
    assert all(r["winner"] >= 0 for rec in recs for r in rec)
    from mpc_gpu.episodes import refill_schedule
    for slots in (4, 2):                                          # what the GPU test asks of steps_run can hold
        assert refill_schedule(lengths, slots)["steps"] < d["max_iter"] * -(-d["count"] // slots)
