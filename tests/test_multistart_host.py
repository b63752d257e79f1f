"""The multi-start solve without a GPU: the two prototypes (header, binding, argument validation on a null handle), the pure helpers of
mpc_gpu.multistart, the numpy selection rule on hand-made tables, and the ORACLE-ALONE CONDITIONS the GPU tests (test_gpu_multistart.py) rely on, stated
as asserts:

  1. every candidate of every parity scene ends with oracle status 0 (at every iteration run);
  2. how far the selection is from going the other way is a relative cost gap >= 1e-4 (multistart_cases.gap: winner against runner-up, and the margin's
     threshold where it decides) -- the cost parity tolerance is 1e-8 relative, so four orders remain and GPU and oracle cannot pick different members;
  3. in at least one scene the winner is not member 0 and costs less than half of member 0 (the feature does something);
  4. 1 and 2 hold on every control step of the lockstep scenes, the oracle driving itself.
A scene that fails a condition is to be replaced, not the threshold lowered.  The figures are printed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import multistart_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpc_gpu.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/mpc_gpu.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _ctype_of(arg):
    if "*" in arg:
        return C.c_void_p
    return {"int": C.c_int, "double": C.c_double}[arg.split()[0]]


@pytest.mark.parametrize("name, count", [("mpc_seed_guesses_dev", 10), ("mpc_select_best_dev", 14)])
def test_header_and_binding_agree_on_the_prototypes(lib, name, count):
    args = _prototype(name)
    assert len(args) == count, args
    res, bound = lib.SYMBOLS[name]
    assert res is C.c_int and bound == [_ctype_of(a) for a in args], (args, bound)
    assert hasattr(C.CDLL(lib.LIB_PATH), name)


def test_abi_version_stays_seven_and_the_flag_is_mirrored(lib):
    hdr = open(os.path.join(ROOT, "include", "mpc_gpu.h")).read()
    assert int(re.search(r"#define\s+MPC_ABI_VERSION\s+(\d+)", hdr).group(1)) == 7 == lib.ABI_VERSION == lib.lib().mpc_abi_version()
    assert int(re.search(r"#define\s+MPC_SELECT_BROADCAST\s+(\d+)", hdr).group(1)) == lib.SELECT_BROADCAST == 1


def test_a_null_handle_is_an_argument_error(lib):
    L = lib.lib()
    assert L.mpc_seed_guesses_dev(None, 1, 5, None, None, None, 0, None, None, None) == lib.MPC_ERR_ARG
    assert b"null handle" in L.mpc_last_error()
    assert L.mpc_select_best_dev(None, 1, 5, None, None, 0.0, 0, None, None, None, None, None, None, None) == lib.MPC_ERR_ARG
    assert b"null handle" in L.mpc_last_error()


# ---------------------------------------------------------------------------------------------------------------- the Python helpers
def test_the_helpers_reject_bad_offsets_margins_and_shapes():
    from mpc_gpu import multistart as ms
    assert ms.check_offsets(mc.OFFSETS).tolist() == list(mc.OFFSETS) and ms.DEFAULT_OFFSETS == mc.OFFSETS
    assert ms.check_offsets([1.5]).shape == (1,) and ms.check_offsets(np.zeros(64)).shape == (64,)
    for bad in ([], np.zeros(65), np.zeros((2, 3)), 2.5, [0.0, np.nan], [0.0, np.inf]):
        with pytest.raises(ValueError):
            ms.check_offsets(bad)
    assert ms.check_margin(0) == 0.0 and ms.check_margin(0.25) == 0.25
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ms.check_margin(bad)
    assert ms.check_scenarios(3, 5) == 3
    for G, K in ((0, 5), (-1, 5), (3, 0), (3, 65)):
        with pytest.raises(ValueError):
            ms.check_scenarios(G, K)
    x0, obst, goal = np.zeros((3, 5)), np.zeros((3, 2, 4)), np.zeros((3, 2))
    ms.check_group_shapes(3, 2, x0, obst, goal)
    for bad in ((np.zeros((3, 4)), obst, goal), (np.zeros((15, 5)), obst, goal), (x0, np.zeros((3, 3, 4)), goal), (x0, np.zeros((3, 21, 2, 2)), goal),
                (x0, obst, np.zeros((3, 3))), (x0, obst, np.zeros(2)), (np.zeros(5), obst, goal)):
        with pytest.raises(ValueError):
            ms.check_group_shapes(3, 2, *bad)
    r = ms.replicate(np.arange(6).reshape(3, 2), 4)
    assert r.shape == (12, 2) and r.flags["C_CONTIGUOUS"] and all((r[g * 4 + k] == [2 * g, 2 * g + 1]).all() for g in range(3) for k in range(4))


def test_multistart_is_exported():
    import mpc_gpu
    assert mpc_gpu.MultiStartMpc is mpc_gpu.multistart.MultiStartMpc and "MultiStartMpc" in mpc_gpu.__all__


# ---------------------------------------------------------------------------------------------------------------- the guess family in numpy
def test_the_numpy_guess_family_is_what_the_header_defines():
    x0, goal, _ = mc.scene("B")
    N = 20
    X, U = mc.guesses(x0, goal, mc.OFFSETS, N)
    assert X.shape == (mc.K, N + 1, 5) and U.shape == (mc.K, N, 2) and not U.any()
    assert (X[:, 0] == x0).all() and not X[:, 1:, 3:].any()
    assert np.abs(X[:, N, :2] - goal).max() < 1e-14                                     # every member ends on the goal
    d = goal - x0[:2]
    n = np.array([-d[1], d[0]]) / np.linalg.norm(d)
    mid = X[:, N // 2, :2] - (x0[:2] + 0.5 * d)                                         # ... and is a offsets[k] to the LEFT of the line at its middle
    assert np.abs(mid @ n - np.array(mc.OFFSETS)).max() < 1e-14 and np.abs(mid @ d).max() < 1e-13
    assert np.abs(X[0, 1:, 2] - np.arctan2(d[1], d[0])).max() < 1e-15                   # the straight member heads along the line (stage 0 is x0)
    # headings follow the path: the finite-difference direction of the positions is the tangent at the midpoint to O(1 / N^2)
    for k in range(mc.K):
        seg = X[k, 2:, :2] - X[k, 1:-1, :2]
        mid_heading = 0.5 * (X[k, 2:, 2] + X[k, 1:-1, 2])
        err = np.angle(np.exp(1j * (np.arctan2(seg[:, 1], seg[:, 0]) - mid_heading)))
        assert np.abs(err).max() < 0.02, (k, np.abs(err).max())
    # the wrap keeps every heading within half a turn of psi0, whatever psi0 is
    for psi in (-9.0, -3.0, 0.0, 3.1, 7.5):
        xs = x0.copy(); xs[2] = psi
        Xw, _ = mc.guesses(xs, goal, mc.OFFSETS, N)
        assert np.abs(Xw[:, 1:, 2] - psi).max() <= np.pi + 1e-12
        assert np.abs(np.angle(np.exp(1j * (Xw[:, 1:, 2] - X[:, 1:, 2])))).max() < 1e-12
    # a robot on its goal: the plain reset guess (v and omega of stage 0 are zero there, as mpc_reset_guess writes them)
    xs = np.array([1.0, 2.0, 0.3, 0.7, -0.2])
    Xr, Ur = mc.guesses(xs, xs[:2] + 1e-10, mc.OFFSETS, 7)
    assert (Xr[:, :, :3] == xs[:3]).all() and not Xr[:, :, 3:].any() and not Ur.any()
    # non-finite inputs propagate
    xs = x0.copy(); xs[1] = np.nan
    assert np.isnan(mc.guesses(xs, goal, mc.OFFSETS, 5)[0][:, :, 1]).all()


# ---------------------------------------------------------------------------------------------------------------- the selection rule in numpy
@pytest.mark.parametrize("name, cost, status, margin, winner", mc.HAND, ids=[h[0] for h in mc.HAND])
def test_the_numpy_selection_rule_on_hand_made_tables(name, cost, status, margin, winner):
    w, c = mc.select(cost, status, margin)
    assert w == winner
    assert (c == np.inf) if winner < 0 else (c == cost[winner])
    # restated: nobody eligible is strictly cheaper than the winner unless the margin kept member 0, and nobody equally cheap sits below it
    ok = mc.eligible(cost, status)
    if winner >= 0:
        assert ok[winner]
        kept = margin > 0 and winner == 0 and ok[0]
        for k in np.nonzero(ok)[0]:
            if kept:
                assert not (cost[k] < (1.0 - margin) * cost[0])
            else:
                assert cost[k] > cost[winner] or (cost[k] == cost[winner] and k >= winner)
    else:
        assert not ok.any()


def test_the_hand_made_tables_cover_the_issue_list_and_group_form():
    names = " ".join(h[0] for h in mc.HAND)
    for word in ("tie", "NaN", "-inf", "+inf", "status 4", "no eligible", "margin kept", "margin beaten"):
        assert word in names, word
    upper = 0
    for Kt in (1, 2, 5, 64):
        for margin, cost, status in mc.hand_table(Kt):
            assert cost.shape == status.shape and cost.shape[1] == Kt
            u0 = np.arange(cost.size * 2, dtype=np.float64).reshape(cost.shape + (2,))
            w, c, b = mc.select_groups(cost, status, margin, u0)
            assert w.dtype == np.int32 and ((w >= -1) & (w < Kt)).all()
            for g in range(len(w)):
                assert (w[g], c[g]) == mc.select(cost[g], status[g], margin)
                assert (b[g] == (u0[g, w[g]] if w[g] >= 0 else 0.0)).all()
            if Kt == 5:
                assert w.tolist() == [h[4] for h in mc.HAND if h[3] == margin]
            if Kt == 64:      # the padding wins only where none of the five is eligible, and then in the upper half of the wavefront
                five = np.array([h[4] for h in mc.HAND if h[3] == margin])
                assert ((w == five) | ((five < 0) & (w == 63))).all()
                upper += int((w == 63).sum())
    assert upper >= 2


# ---------------------------------------------------------------------------------------------------------------- the oracle-alone conditions
def _conditions(tag, r):
    print(f"MULTISTART-HOST {tag}: cost {['%.6g' % c for c in r['cost']]} status {r['status'].tolist()} interior-point iterations {r['iters'].tolist()} "
          f"winner {r['winner']} gap {r['gap']:.3e}")
    assert (r["status"] == 0).all(), (tag, r["status"])
    assert np.isfinite(r["cost"]).all()
    assert r["gap"] >= mc.MIN_GAP, (tag, r["gap"])


@pytest.mark.parametrize("case", mc.PARITY, ids=mc.PARITY_IDS)
def test_every_parity_scene_meets_the_conditions_on_the_oracle(orc, case):
    name, N, Tf, it = case
    r = mc.oracle_group(orc, name, N, Tf, it)
    _conditions(f"{name} N={N} iterations={it}", r)
    assert (r["sqp_iters"] == it).all()
    # every iteration run, not only the last, ended with status 0: run the first it - 1 alone
    for j in range(1, it):
        assert (mc.oracle_group(orc, name, N, Tf, j)["status"] == 0).all(), (name, j)


def test_multi_start_finds_a_better_family_in_some_scene(orc):
    found = []
    for name, N, Tf, it in mc.PARITY:
        r = mc.oracle_group(orc, name, N, Tf, it)
        if r["winner"] != 0 and r["cost"][r["winner"]] < 0.5 * r["cost"][0]:
            found.append((name, N, it, r["winner"], r["cost"][0] / r["cost"][r["winner"]]))
    print("MULTISTART-HOST scenes where a member other than 0 costs less than half of member 0 (scene, N, iterations, winner, ratio):", found)
    assert found


@pytest.mark.parametrize("case", mc.LOCKSTEP, ids=mc.LOCKSTEP_IDS)
def test_the_lockstep_scenes_meet_the_conditions_on_every_step(orc, case):
    name, margin = case
    recs = mc.oracle_loop(orc, name, margin)
    assert len(recs) == mc.LOCKSTEP_STEPS
    for k, r in enumerate(recs):
        _conditions(f"lockstep {name} margin {margin} step {k}", r)
    winners = [r["winner"] for r in recs]
    print(f"MULTISTART-HOST lockstep {name} margin {margin}: winners {winners}")
    assert winners[0] != 0                       # the loop starts in a family the straight line does not reach


def test_the_margin_case_consults_the_margin(orc):
    """the lockstep case with incumbent_margin = 0.1 is there to exercise the margin in the loop: on at least one of its steps member 0 is eligible and
    not the least, so that the compare against (1 - m) cost[0] decides (both of its outcomes are in the hand-made tables; which one the scene takes is
    recorded).  How close that compare is enters multistart_cases.gap, which the conditions above bound."""
    name, margin = next(c for c in mc.LOCKSTEP if c[1] > 0)
    assert margin == 0.1
    recs = mc.oracle_loop(orc, name, margin)
    plain = [mc.select(r["cost"], r["status"], 0.0)[0] for r in recs]
    kept = [r["winner"] for r in recs]
    consulted = [k for k, r in enumerate(recs) if plain[k] > 0 and mc.eligible(r["cost"], r["status"])[0]]
    ratio = [float(recs[k]["cost"][plain[k]] / recs[k]["cost"][0]) for k in consulted]
    print(f"MULTISTART-HOST lockstep {name}: winners with margin {margin} {kept}, the plain rule on the same tables {plain}; the margin decided on steps "
          f"{consulted} with challenger / incumbent cost {['%.4f' % r for r in ratio]} (kept from {1.0 - margin} on)")
    assert consulted
