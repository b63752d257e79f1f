"""The rollout merit without a GPU: the prototype (header, binding, argument validation without a device), check_select_by, and the ORACLE-ALONE
CONDITIONS that make the GPU comparisons of test_gpu_rollout_merit.py sharp, stated as asserts:

  1. the numpy restatement of the objective (rollout_merit_cases.merit_np, used where the oracle has no switch) equals oracle.cost on the default-feature
     cases to 1e-12 relative;
  2. on a dynamically feasible iterate (X = X^r) the merit IS oracle.cost(X, U) and the defect is <= 1e-13;
  3. every parity case has an instance with defect > 1e-3 and |merit - cost(X, U)| > 1e-4 relative -- a kernel that scored the given X instead of the
     rollout fails the 1e-8 comparison by four orders;
  4. the margins of the parity cases include a negative and a positive one, each >= 1e-3 from 0;
  5. the bounds case (a small per-instance speed bound) has boxviol > 1e-3, and every feature case moves its figure by more than 1e-4 relative;
  6. among the multi-start scenes at least one has different cost and merit argmins after one RTI iteration of the oracle, and every selection by merit
     -- every step of the lockstep scenes included -- is a relative gap >= 1e-4 from going the other way (test_multistart_host.py's condition).
A case that fails a condition is to be replaced, not the threshold lowered.  The figures are printed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import multistart_cases as mc
import rollout_merit_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mpc_rollout_merit_dev"


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
def test_header_and_binding_agree_on_the_prototype(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpc_gpu.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{NAME} is not declared in include/mpc_gpu.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert len(args) == 14, args
    want = [C.c_void_p if "*" in a else {"int": C.c_int, "double": C.c_double}[a.split()[0]] for a in args]
    res, bound = lib.SYMBOLS[NAME]
    assert res is C.c_int and bound == want, (args, bound)
    assert hasattr(C.CDLL(lib.LIB_PATH), NAME)
    hdr = open(os.path.join(ROOT, "include", "mpc_gpu.h")).read()
    assert int(re.search(r"#define\s+MPC_ABI_VERSION\s+(\d+)", hdr).group(1)) == 7 == lib.ABI_VERSION == lib.lib().mpc_abi_version()
    assert "get_residuals()[1]" in hdr      # the header says what the defect stands in for


def test_argument_validation_without_a_device(lib):
    L, ERR = lib.lib(), lib.MPC_ERR_ARG
    p = C.c_void_p(8)      # a non-null pointer that is never followed: every call below is refused before anything is read or launched
    call = lambda h=None, batch=1, members=1, x0=p, P=p, goal=p, X=p, U=p, merit=p, defect=None, margin=None, boxviol=None, Xr=None: \
        L.mpc_rollout_merit_dev(h, batch, members, x0, P, goal, X, U, merit, defect, margin, boxviol, Xr, None)
    for kw, word in ((dict(batch=0), b"batch"), (dict(batch=-3), b"batch"), (dict(members=0), b"members"), (dict(members=-1), b"members"),
                     (dict(merit=None), b"no output"), (dict(X=None, defect=p), b"d_defect needs d_X"), (dict(x0=None), b"null device pointer"),
                     (dict(P=None), b"null device pointer"), (dict(goal=None), b"null device pointer"), (dict(U=None), b"null device pointer"),
                     (dict(), b"null handle"), (dict(X=None), b"null handle"), (dict(merit=None, Xr=p), b"null handle")):
        assert call(**kw) == ERR and word in L.mpc_last_error(), (kw, L.mpc_last_error())


def test_check_select_by():
    from mpc_gpu import multistart as ms
    assert ms.check_select_by("cost") == "cost" and ms.check_select_by("rollout") == "rollout" and ms.SELECT_BY == ("cost", "rollout")
    for bad in ("", "Cost", "merit", None, 0, 1.0, ("cost",), b"cost"):
        with pytest.raises(ValueError):
            ms.check_select_by(bad)
    with pytest.raises(ValueError):          # ... and the constructor judges it before it touches a device
        ms.MultiStartMpc(select_by="best")


# ---------------------------------------------------------------------------------------------------------------- the oracle-alone conditions
def test_the_restatement_is_the_oracles_cost_on_the_default_cases(orc):
    worst = 0.0
    for shp in rc.SHAPES:
        c = rc.case(orc, *shp)
        for b in range(shp[2]):
            g = b // shp[3]
            for X in (c["Xr"][b], c["X"][b]):
                a, o = rc.merit_np(c["cfg"], c["x0"][g], c["P"][g], c["goal"][g], X, c["U"][b]), orc.cost(c["cfg"], c["x0"][g], c["P"][g], c["goal"][g], X, c["U"][b])
                worst = max(worst, abs(a - o) / abs(o))
        assert np.allclose(rc.builtin_alpha(c["cfg"], c["x0"][0], c["goal"][0]), orc.slack_alpha(c["cfg"], c["x0"][0], c["goal"][0]), rtol=1e-12, atol=0.0)
    print(f"ROLLOUT-HOST restatement against oracle.cost: worst relative difference {worst:.3e}")
    assert worst <= 1e-12
    for name in ("params", "mask"):          # ... and where the oracle has the switch too, the two agree with the feature on
        f = rc.feature(orc, name)
        assert rc.rel_change(f["merit"], f["merit_np"]).max() <= 1e-12


@pytest.mark.parametrize("shp", rc.SHAPES, ids=rc.SHAPE_IDS)
def test_every_parity_case_is_sharp(orc, shp):
    N, no, B, m = shp
    c = rc.case(orc, *shp)
    # a dynamically feasible iterate: the merit is the cost of the iterate, and it has no defect
    for b in range(B):
        g = b // m
        assert rc.defect(orc, c["x0"][g], c["Xr"][b], c["U"][b], c["dt"]) <= 1e-13
        assert c["merit"][b] == orc.cost(c["cfg"], c["x0"][g], c["P"][g], c["goal"][g], c["Xr"][b], c["U"][b])
    rel = rc.rel_change(c["merit"], c["cost_X"])
    print(f"ROLLOUT-HOST N={N} n_obst={no} batch={B} members={m}: defect {c['defect'].min():.2e} .. {c['defect'].max():.2e}, |merit - cost(X, U)| / merit up to "
          f"{rel.max():.2e}, margin {c['margin'].min():.3f} .. {c['margin'].max():.3f}, boxviol up to {c['boxviol'].max():.3f}, |X^r| up to {np.abs(c['Xr']).max():.1f}")
    assert ((c["defect"] > 1e-3) & (rel > 1e-4)).any()
    assert np.isfinite(c["merit"]).all() and np.abs(c["Xr"]).max() < 100.0      # (the 1e-10 bound on X^r is argued for entries of this size)
    if m > 1:      # the members of a group share a row and differ in U: their merits differ
        assert len(set(c["merit"][:m].tolist())) == m


def test_the_margins_have_both_signs_and_the_boxes_are_violated_somewhere(orc):
    mar = np.concatenate([rc.case(orc, *shp)["margin"] for shp in rc.SHAPES])
    box = np.concatenate([rc.case(orc, *shp)["boxviol"] for shp in rc.SHAPES])
    assert (mar <= -1e-3).any() and (mar >= 1e-3).any() and np.isfinite(mar).all()
    assert (box > 1e-3).any() and (box == 0.0).any()


@pytest.mark.parametrize("name", rc.FEATURES)
def test_every_feature_case_moves_its_figure(orc, name):
    N, no, B, m = rc.FEATURE_SHAPE
    base, f = rc.case(orc, N, no, B, m), rc.feature(orc, name)
    ch = {k: rc.rel_change(f[k], base[k]) for k in ("merit", "margin", "boxviol")}
    print(f"ROLLOUT-HOST feature {name}: relative change of merit {ch['merit'].tolist()}, margin {ch['margin'].tolist()}, boxviol {f['boxviol'].tolist()}")
    moved = {"alpha": ("merit",), "reference": ("merit",), "params": ("merit", "margin"), "mask": ("merit", "margin"), "bounds": ("boxviol",)}[name]
    for k in moved:
        assert ch[k].max() > rc.MIN_EFFECT, (name, k)
    for k in set(ch) - set(moved):
        assert np.array_equal(f[k], base[k])
    if name == "bounds":
        assert (f["boxviol"] > 1e-3).all() and not base["boxviol"].any()


def test_the_multi_start_scenes_meet_the_conditions_on_the_oracle(orc):
    differ = []
    for name in rc.MS_SCENES:
        for margin in sorted({0.0} | ({rc.MS_MARGIN_SCENE[1]} if name == rc.MS_MARGIN_SCENE[0] else set())):
            r = rc.ms_group(orc, name, margin)
            print(f"ROLLOUT-HOST scene {name} margin {margin}: cost {['%.6g' % c for c in r['cost']]} merit {['%.6g' % c for c in r['merit']]} defect "
                  f"{['%.3f' % c for c in r['defect']]} margin {['%.3f' % c for c in r['margin']]} winner by cost {r['winner_by_cost']} by merit {r['winner']} gap {r['gap']:.3e}")
            assert (r["status"] == 0).all() and np.isfinite(r["merit"]).all()
            assert r["gap"] >= mc.MIN_GAP, (name, r["gap"])
            if margin == 0.0 and int(np.argmin(r["cost"])) != int(np.argmin(r["merit"])):
                differ.append(name)
    assert differ      # the two rules do not pick the same member everywhere: the selection by merit is visible


@pytest.mark.parametrize("case", rc.MS_LOCKSTEP, ids=rc.MS_LOCKSTEP_IDS)
def test_the_lockstep_scenes_meet_the_conditions_on_every_step(orc, case):
    name, margin = case
    recs = rc.ms_loop(orc, name, margin)
    assert len(recs) == rc.MS_STEPS
    for k, r in enumerate(recs):
        print(f"ROLLOUT-HOST lockstep {name} margin {margin} step {k}: winner by merit {r['winner']} by cost {r['winner_by_cost']} gap {r['gap']:.3e} status {r['status'].tolist()}")
        assert (r["status"] == 0).all() and np.isfinite(r["merit"]).all()
        assert r["gap"] >= mc.MIN_GAP, (name, k, r["gap"])
