"""The group control step and its episode driver without a GPU: the prototype (header, binding, struct mirror, the argument errors that need no device),
the driver's argument checks (they raise before a handle exists), the numpy restatement of the six points (multistart_episode_cases.tail) on its
degenerate ends, and the ORACLE-ALONE CONDITIONS test_gpu_multistart_episodes.py relies on, stated as asserts for the scenes and control steps it runs:

  1. every selection is a relative gap >= 1e-4 (multistart_cases.MIN_GAP) from going the other way;
  2. no bookkeeping threshold (goal tolerance, arena edge, margin 0) lies within 1e-6 of the value tested against it.
A scene that fails a condition is to be replaced, not the threshold lowered.  The figures are printed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import multistart_cases as mc
import multistart_episode_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mpc_group_step_dev"


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


@pytest.fixture(scope="module")
def lib(built):
    from mpc_gpu import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpc_gpu.h")).read(), flags=re.S)


def test_header_and_binding_agree_on_the_prototype_and_the_struct(lib):
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{NAME} is not declared in include/mpc_gpu.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert len(args) == 19, args
    want = [C.POINTER(lib.GroupStepOut) if "mpc_group_step_out" in a else (C.c_void_p if "*" in a else {"int": C.c_int, "double": C.c_double}[a.split()[0]]) for a in args]
    res, bound = lib.SYMBOLS[NAME]
    assert res is C.c_int and bound == want, (args, bound)
    assert hasattr(C.CDLL(lib.LIB_PATH), NAME)
    body = re.search(r"typedef struct mpc_group_step_out\s*\{(.*?)\}\s*mpc_group_step_out\s*;", _header(), flags=re.S).group(1)
    fields = [f.strip().lstrip("*") for decl in body.split(";") if decl.strip() for f in decl.split("*", 1)[1].split(",")]
    assert fields == [n for n, _ in lib.GroupStepOut._fields_], fields
    assert C.sizeof(lib.GroupStepOut) == 8 * len(fields)
    hdr = open(os.path.join(ROOT, "include", "mpc_gpu.h")).read()
    assert int(re.search(r"#define\s+MPC_GROUP_MARGIN_ALL\s+(\d+)", hdr).group(1)) == lib.GROUP_MARGIN_ALL == 1
    assert int(re.search(r"#define\s+MPC_ABI_VERSION\s+(\d+)", hdr).group(1)) == 7 == lib.ABI_VERSION == lib.lib().mpc_abi_version()


def test_a_null_handle_and_a_bad_member_count_are_argument_errors(lib):
    L = lib.lib()
    out = lib.GroupStepOut()
    call = lambda h, G, K, m=0.0, f=0: L.mpc_group_step_dev(h, G, K, None, None, None, m, f, None, None, None, None, None, 0.1, 2.0, None, None, out, None)
    assert call(None, 1, 5) == lib.MPC_ERR_ARG and b"null handle" in L.mpc_last_error()
    assert call(None, 1, 0) == lib.MPC_ERR_ARG and call(None, 1, 65) == lib.MPC_ERR_ARG and call(None, -1, 5) == lib.MPC_ERR_ARG


# ---------------------------------------------------------------------------------------------------------------- the driver's argument checks
def test_the_driver_refuses_bad_arguments_before_any_device_use(monkeypatch):
    import mpc_gpu
    from mpc_gpu import multistart as ms
    assert mpc_gpu.run_multistart_episodes is ms.run_multistart_episodes and "run_multistart_episodes" in mpc_gpu.__all__

    def no_handle(*a, **k):
        raise AssertionError("a handle was made before the arguments were checked")
    monkeypatch.setattr(ms, "MultiStartMpc", type("Refuse", (), {"__init__": no_handle}))
    x0, goal, obst = np.zeros((3, 5)), np.zeros(2), np.zeros((3, 2, 4))
    ok = ms.episode_arguments(x0, goal, obst, noise=np.zeros((400, 3, 2, 2)))
    assert (ok["G"], ok["K"], ok["n_obst"]) == (3, 5, 2) and ok["goal"].shape == (3, 2) and ok["scenario"] is None
    assert ms.episode_arguments(x0, goal, "RANDOM")["noise"] == "reference" and ms.episode_arguments(x0, goal, "EDGE", random_move=False)["noise"] is None
    bad = [dict(x0=np.zeros((3, 4))), dict(x0=np.zeros(5)), dict(x0=np.zeros((0, 5))), dict(goal=np.zeros((2, 2))), dict(obst=np.zeros((2, 2, 4))),
           dict(obst=np.zeros((3, 2, 3))), dict(obst=np.zeros((3, 33, 4))), dict(obst="MIDDLE"), dict(obst="RANDOM", n_obst=0), dict(obst="RANDOM", n_obst=33),
           dict(offsets=[]), dict(offsets=np.zeros(65)), dict(offsets=[0.0, np.nan]), dict(incumbent_margin=1.0), dict(incumbent_margin=-0.1),
           dict(select_by="merit"), dict(max_iter=0), dict(max_iter=2.5), dict(first_seed=-1), dict(first_seed=2 ** 32), dict(noise=np.zeros((5, 3, 2, 2))),
           dict(noise=np.zeros((400, 4, 2, 2))), dict(noise="reference"), dict(sqp=3), dict(r_safe=np.ones((2, 2))), dict(r_hit=-np.ones(3)),
           dict(active=np.ones((3, 3), bool)), dict(active=np.ones((3, 2))), dict(solver=object())]
    for kw in bad:
        args = dict(x0=x0, goal=goal, obst=obst)
        args.update(kw)
        with pytest.raises(ValueError):
            ms.run_multistart_episodes(args.pop("x0"), args.pop("goal"), args.pop("obst"), **args)


# ---------------------------------------------------------------------------------------------------------------- the numpy restatement on its ends
def _group(orc, K, N=8, no=2, seed=0):
    rng = np.random.default_rng(seed)
    cfg = orc.config(N, no, 0.1 * N)
    return dict(cfg=cfg, key=rng.uniform(1, 9, K), status=np.zeros(K, np.int32), u0=rng.uniform(-2, 2, (K, 2)), x=np.array([-3.0, 1.0, 0.2, 1.0, 0.1]),
                obst=np.array([[0.0, 0.5, 0.3, -0.2], [4.0, -4.0, 0.0, 0.5]])[:no], goal=np.array([5.0, 2.0]), X=rng.uniform(-5, 5, (K, N + 1, 5)),
                U=rng.uniform(-2, 2, (K, N, 2)), noise=rng.standard_normal((no, 2)))


def _tail(orc, g, offsets, margin=0.0, book=None, **kw):
    return ec.tail(orc, g["cfg"], offsets, margin, g["key"], g["status"], g["u0"], g["x"], g["obst"], g["goal"], g["X"], g["U"], g["noise"],
                   ec.new_book() if book is None else book, **kw)


def test_the_restatement_with_one_member(orc):
    g = _group(orc, 1)
    t = _tail(orc, g, (0.0,))
    assert t["winner"] == 0 and t["best_key"] == g["key"][0] and np.array_equal(t["best_u0"], g["u0"][0])
    assert np.array_equal(t["x"], orc.dynamics(g["x"], g["u0"][0], 0.1)[0])
    Xs, Us = orc.shift(g["cfg"], g["X"][0], g["U"][0])
    assert np.array_equal(t["X"][0], Xs) and np.array_equal(t["U"][0], Us) and not t["U"][0, -1].any() and np.array_equal(t["X"][0, -1], g["X"][0, -1])
    assert t["book"] == dict(min_margin=t["book"]["min_margin"], flags=0, steps=1, lost=0, switched=0) and np.isfinite(t["book"]["min_margin"])
    assert t["member_x"].shape == (1, 5) and np.array_equal(t["member_x"][0], t["x"]) and t["member_flags"].tolist() == [0]


def test_the_restatement_without_an_eligible_member(orc):
    g = _group(orc, 3)
    g["status"][:] = 4
    t = _tail(orc, g, (0.0, 2.5, -2.5), margin=0.25)
    assert t["winner"] == -1 and np.isinf(t["best_key"]) and not t["best_u0"].any()
    assert np.array_equal(t["x"], orc.dynamics(g["x"], np.zeros(2), 0.1)[0])                       # it coasts
    Xg, Ug = mc.guesses(t["x"], g["goal"], (0.0, 2.5, -2.5), g["cfg"].N)
    assert np.array_equal(t["X"], Xg) and np.array_equal(t["U"], Ug)                               # all members seeded, member 0 included
    assert t["book"]["lost"] == 1 and t["book"]["switched"] == 0 and t["book"]["steps"] == 1
    g["status"][:] = 0; g["key"][:] = [5.0, 3.0, 4.0]
    assert _tail(orc, g, (0.0, 2.5, -2.5))["book"]["switched"] == 1 and _tail(orc, g, (0.0, 2.5, -2.5), margin=0.5)["winner"] == 0


def test_the_restatement_on_the_goal_at_the_walls_and_in_an_obstacle(orc):
    g = _group(orc, 2)
    g["u0"][:] = 0.0; g["x"] = np.array([4.95, 1.9, 0.2, 0.0, 0.0])
    t = _tail(orc, g, (2.5, -2.5))
    assert t["book"]["flags"] == 1 and t["book"]["steps"] == 0 and t["member_flags"].tolist() == [1, 1]
    g["x"] = np.array([7.95, 0.0, 0.0, 2.0, 0.0])
    assert _tail(orc, g, (2.5, -2.5))["book"]["flags"] == 2
    g["x"] = np.array([0.0, 0.0, 0.0, 0.0, 0.0])                                                   # obstacle 0 is half a metre away
    t = _tail(orc, g, (2.5, -2.5))
    assert t["book"]["flags"] == 4 and t["book"]["min_margin"] < 0 and t["book"]["steps"] == 1
    assert _tail(orc, g, (2.5, -2.5), active=[False, True])["book"]["flags"] == 0                  # absent: not counted ...
    assert _tail(orc, g, (2.5, -2.5), active=[False, True], margin_all=True)["book"]["flags"] == 4      # ... unless every obstacle counts
    assert _tail(orc, g, (2.5, -2.5), r_hit=[0.1, 0.1])["book"]["flags"] == 0 and _tail(orc, g, (2.5, -2.5), r_hit=[0.1, 9.0])["book"]["flags"] == 4
    assert _tail(orc, g, (2.5, -2.5), active=[False, False])["book"]["min_margin"] == np.inf
    keep = _tail(orc, g, (2.5, -2.5), book=dict(min_margin=-0.5, flags=4, steps=7, lost=2, switched=3), active=[False, True])["book"]
    assert keep["min_margin"] == -0.5 and keep["flags"] == 4 and keep["steps"] == 8 and keep["lost"] == 2      # the running minimum and its flag stay


def test_the_restatement_leaves_an_idle_group_as_it_is(orc):
    g = _group(orc, 3)
    book = dict(min_margin=0.7, flags=1, steps=5, lost=1, switched=2)
    t = _tail(orc, g, (0.0, 2.5, -2.5), book=book)
    assert t["idle"] and t["book"] == book
    for k in ("x", "obst", "X", "U"):
        assert np.array_equal(t[k], g[k])
    assert set(t) == {"idle", "x", "obst", "X", "U", "book"}


# ---------------------------------------------------------------------------------------------------------------- the oracle-alone conditions
def _conditions(tag, groups, steps):
    for g, recs in enumerate(groups):
        assert len(recs) == steps, (tag, g, len(recs))
        gaps, nears = [r["gap"] for r in recs], [r["near"] for r in recs]
        print(f"MULTISTART-EPISODES-HOST {tag} group {g}: winners {[r['winner'] for r in recs]} least gap {min(gaps):.3e} least distance from a threshold "
              f"{min(nears):.3e} flags {[r['book']['flags'] for r in recs]}")
        assert min(gaps) >= mc.MIN_GAP, (tag, g, gaps)
        assert min(nears) >= ec.MIN_NEAR, (tag, g, nears)
        assert all(r["winner"] >= 0 for r in recs), (tag, g)


@pytest.mark.parametrize("shape", ec.SHAPES, ids=ec.SHAPE_IDS)
def test_the_lockstep_scenes_meet_the_conditions_on_every_step(orc, shape):
    _conditions("lockstep %s" % (shape,), ec.oracle_loop(orc, shape), ec.STEPS)


def test_the_driver_episodes_meet_the_conditions_on_every_step(orc):
    from mpc_gpu import world
    _conditions("driver", ec.oracle_driver_loop(orc, world), ec.DRIVER["max_iter"])
