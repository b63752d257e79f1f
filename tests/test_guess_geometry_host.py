"""The guess family from geometry without a GPU: the numpy restatement of the rule (guess_geometry_cases.amplitudes) on hand-computed answers; the
agreement of header and binding on the two entry points; the refusals of check_guess_geometry and of the drivers, which come before a handle exists; and
the NUMPY-ALONE CONDITIONS test_gpu_guess_geometry.py relies on, stated as asserts:

  1. every scene the GPU tests compare at a tolerance has a decision gap >= 1e-6 (guess_geometry_cases: the least distance of the rule's inputs from a
     point where its answer jumps); scene B as it stands and scene A at lead = 1 are shown NOT to qualify (gap 0), which is why they are not used;
  2. along the oracle-driven closed loop of the GPU lockstep test every control step's gap is >= 1e-6, the selection's cost gap >= 1e-4 and every
     candidate is solved (status 0 or 2).
A scene that fails a condition is to be replaced, not the threshold lowered.  The figures are printed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import guess_geometry_cases as gc
import multistart_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_GAP = 1e-6


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


@pytest.fixture(scope="module")
def lib(built):
    from mpc_gpu import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------------------- hand-computed answers
def _hand(x0, goal, obst, offsets, **kw):
    return gc.amplitudes(x0, goal, obst, offsets, **dict(gc.HAND, **kw))


def test_scene_a_by_hand():
    """the obstacle at (0, 0.2) sits at s = 0.5 (w = 1), c = 0.2, R = 2.5: left 2.7, right -2.3; the other two are 3 m off the line (|c| = 3 >= 2.5)"""
    x0, goal, obst = mc.scene("A")
    a, info = _hand(x0, goal, obst, mc.OFFSETS)
    assert info["blocks"].tolist() == [True, False, False] and info["order"] == [0]
    assert np.allclose(a, gc.SCENE_A_WANT, rtol=0, atol=1e-15) and a[0] == 0.0 and a[3] == 5.0 and a[4] == -5.0


def test_the_tie_and_clamp_scene_by_hand():
    """nearest first (obstacle 2 at al = 0.5, w = sin(0.05 pi): both amplitudes clamped to +-6), then the exact tie at al = 5 to the lower index
    (obstacle 0: 3, -2; obstacle 1: 2, -3), the last member on its base offset -- exactly, every product being exact"""
    t = gc.TIE
    a, info = _hand(t["x0"], t["goal"], t["obst"], t["offsets"])
    assert info["order"] == [2, 0, 1] and info["blocks"].all()
    assert a.tolist() == list(t["want"])
    assert info["gap"] == 0.0                                     # (the tie: this scene is compared bit for bit, not at a tolerance)


def test_mask_radii_short_line_and_nan():
    x0, goal, obst = mc.scene("A")
    # an absent obstacle does not block: every member keeps its base offset
    a, info = _hand(x0, goal, obst, mc.OFFSETS, active=[False, True, True])
    assert a.tolist() == list(mc.OFFSETS) and not info["blocks"].any()
    # per-obstacle radii: obstacle 0 shrunk below |c| = 0.2 - clearance no longer blocks, obstacle 1 grown over |c| = 3 does (s = 0.7)
    a, info = _hand(x0, goal, obst, mc.OFFSETS, r=[0.05, 3.0, 2.4])
    assert info["blocks"].tolist() == [False, True, False]
    w = np.sin(np.pi * 0.7)
    assert np.allclose(a, [0.0, (-3.0 + 3.1) / w, max((-3.0 - 3.1) / w, -6.0), 5.0, -5.0], rtol=0, atol=1e-14) and a[2] == -6.0
    # L < 1e-9: the base family, whatever stands around
    a, info = _hand([1.0, 2.0, 0.3, 0.0, 0.0], [1.0, 2.0 + 5e-10], [[1.0, 2.0, 0.0, 0.0]] * 3, mc.OFFSETS)
    assert a.tolist() == list(mc.OFFSETS) and info["gap"] == np.inf
    # a NaN obstacle row does not block, the others do as before
    ob = obst.copy(); ob[1] = np.nan
    a, info = _hand(x0, goal, ob, mc.OFFSETS)
    assert info["blocks"].tolist() == [True, False, False] and np.allclose(a, gc.SCENE_A_WANT, rtol=0, atol=1e-15)
    ob = obst.copy(); ob[0, 0] = np.inf
    assert _hand(x0, goal, ob, mc.OFFSETS)[0].tolist() == list(mc.OFFSETS)
    # the lead moves the obstacle along its velocity: obstacle 1 of scene A comes within R after one second (and |c| = R exactly: it does NOT block)
    a, info = _hand(x0, goal, obst, mc.OFFSETS, lead=1.0)
    assert info["blocks"].tolist() == [True, False, False]
    a, info = _hand(x0, goal, obst, mc.OFFSETS, lead=1.5)
    assert info["blocks"].tolist() == [True, True, False] and info["order"] == [0, 1]


def test_more_members_than_candidates_and_fewer():
    """K = 2 takes the first obstacle's left alone; K = 8 with two blockers takes four candidates and keeps the base offsets of members 5 .. 7"""
    x0, goal, obst = gc.scene("C")
    off8 = np.array([0.0, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 4.0])
    a8, info = gc.amplitudes(x0, goal, obst, off8, **gc.GEOM)
    assert len(info["order"]) == 2 and a8[5:].tolist() == off8[5:].tolist() and a8[0] == 0.0
    a2, _ = gc.amplitudes(x0, goal, obst, off8[:2], **gc.GEOM)
    assert a2.tolist() == a8[:2].tolist()
    assert a8[1] > a8[2] and a8[3] > a8[4]                        # left above right for each obstacle


# ---------------------------------------------------------------------------------------------------------------- conditions of the GPU scenes
def test_the_gpu_scenes_are_away_from_every_decision():
    for name, lead in gc.GPU_SCENES:
        x0, goal, obst = gc.scene(name)
        for geom in (dict(gc.GEOM, lead=lead), dict(gc.HAND, lead=lead)):
            a, info = gc.amplitudes(x0, goal, obst, mc.OFFSETS, **geom)
            print(f"GUESS-GEOMETRY scene {name} lead {lead} clearance {geom['clearance']}: blockers {info['order']} amplitudes {a.tolist()} gap {info['gap']:.3g}")
            assert info["gap"] >= MIN_GAP and len(info["order"]) >= 1
    # what is NOT used, and why
    x0, goal, obst = mc.scene("B")
    assert gc.amplitudes(x0, goal, obst, mc.OFFSETS, **gc.GEOM)[1]["gap"] < MIN_GAP             # obstacles 0 and 1 have equal al up to rounding
    x0, goal, obst = mc.scene("A")
    assert gc.amplitudes(x0, goal, obst, mc.OFFSETS, **dict(gc.HAND, lead=1.0))[1]["gap"] < MIN_GAP      # |c| = R exactly


@pytest.mark.parametrize("no", [1, 3, 10, 32])
def test_the_tables_are_away_from_every_decision(no):
    for lead in (0.0, 1.0):
        x, goal, obst = gc.hand_table(7, no, lead)
        a, gaps, nb = gc.group_amplitudes(x, goal, obst, mc.OFFSETS, dict(gc.GEOM, lead=lead))
        print(f"GUESS-GEOMETRY hand table no={no} lead={lead}: blockers {nb.tolist()} least gap {gaps.min():.3g}")
        assert gaps.min() >= MIN_GAP and nb.max() >= 1
    x, goal, obst = gc.random_table(no)
    for K, off in ((5, mc.OFFSETS), (8, np.linspace(-3.5, 3.5, 8))):
        a, gaps, nb = gc.group_amplitudes(x, goal, obst, off, dict(gc.GEOM, lead=gc.RANDOM_LEAD))
        print(f"GUESS-GEOMETRY random table no={no} K={K}: blockers {nb.min()} .. {nb.max()}, least gap {gaps.min():.3g}")
        assert gaps.min() >= MIN_GAP
        if no >= 3:
            assert nb.max() >= 2                                  # (some groups have several blockers: the order and the second pair are exercised)


@pytest.mark.parametrize("case", gc.LOCKSTEP, ids=gc.LOCKSTEP_IDS)
def test_the_lockstep_loop_is_away_from_every_decision(orc, case):
    recs = gc.oracle_loop(orc, *case)
    gaps = [r["gap"] for r in recs]
    print(f"GUESS-GEOMETRY lockstep {case}: winners {[r['winner'] for r in recs[1:]]} rule gaps {['%.3g' % g for g in gaps]} "
          f"selection gaps {['%.3g' % r['select_gap'] for r in recs[1:]]}")
    assert min(gaps) >= MIN_GAP
    for r in recs[1:]:
        assert r["winner"] >= 0 and r["select_gap"] >= mc.MIN_GAP and np.isin(r["status"], (0, 2)).all()
    assert any(not np.array_equal(r["amps"], np.array(mc.OFFSETS)) for r in recs)            # the rule does act along the loop


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpc_gpu.h")).read(), flags=re.S)


def test_header_and_binding_agree_on_the_two_entry_points(lib):
    want_names = {"mpc_set_guess_geometry": ["h", "mode", "clearance", "a_max", "lead"],
                  "mpc_seed_guesses_geom_dev": ["h", "groups", "K", "d_x0", "d_obst", "d_goal", "d_offsets", "keep_first", "d_X", "d_U", "d_offsets_out", "stream"]}
    for name, names in want_names.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
        assert m, f"{name} is not declared in include/mpc_gpu.h"
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert [re.search(r"(\w+)$", a).group(1) for a in args] == names
        want = [C.c_void_p if "*" in a else {"int": C.c_int, "double": C.c_double}[a.split()[0]] for a in args]
        res, bound = lib.SYMBOLS[name]
        assert res is C.c_int and bound == want, (args, bound)
        assert hasattr(C.CDLL(lib.LIB_PATH), name)
    hdr = open(os.path.join(ROOT, "include", "mpc_gpu.h")).read()
    assert int(re.search(r"#define\s+MPC_ABI_VERSION\s+(\d+)", hdr).group(1)) == lib.ABI_VERSION == lib.lib().mpc_abi_version()      # additive


def test_argument_errors_that_need_no_device(lib):
    L = lib.lib()
    assert L.mpc_set_guess_geometry(None, 1, 0.25, 6.0, 0.0) == lib.MPC_ERR_ARG and b"null handle" in L.mpc_last_error()
    assert L.mpc_seed_guesses_geom_dev(None, 1, 1, None, None, None, None, 0, None, None, None, None) == lib.MPC_ERR_ARG and b"null handle" in L.mpc_last_error()


# ---------------------------------------------------------------------------------------------------------------- the Python checks
def test_check_guess_geometry():
    import mpc_gpu
    from mpc_gpu import multistart as ms
    assert mpc_gpu.check_guess_geometry is ms.check_guess_geometry and "check_guess_geometry" in mpc_gpu.__all__
    chk = ms.check_guess_geometry
    assert chk(None) is None and chk(False) is None
    assert chk(True) == dict(clearance=0.25, a_max=6.0, lead=0.0) == ms.GUESS_GEOMETRY_DEFAULTS == gc.GEOM
    assert chk({}) == chk(True) and chk(True) is not ms.GUESS_GEOMETRY_DEFAULTS
    assert chk(dict(lead=0.5)) == dict(clearance=0.25, a_max=6.0, lead=0.5)
    assert chk(dict(clearance=0, a_max=np.float64(3), lead=1)) == dict(clearance=0.0, a_max=3.0, lead=1.0)
    nan, inf = float("nan"), float("inf")
    for bad in (1, "on", [0.25, 6.0, 0.0], dict(margin=0.1), dict(clearance=-0.1), dict(clearance=nan), dict(clearance=inf), dict(a_max=0.0), dict(a_max=-1.0),
                dict(a_max=nan), dict(a_max=inf), dict(lead=-1e-9), dict(lead=nan), dict(lead=inf), dict(lead="1"), dict(a_max=None), dict(clearance=True)):
        with pytest.raises(ValueError, match="guess_geometry"):
            chk(bad)


def test_the_drivers_check_guess_geometry_before_any_device_use(monkeypatch):
    from mpc_gpu import multistart as ms

    def no_handle(*a, **k):
        raise AssertionError("a handle was made before the arguments were checked")
    monkeypatch.setattr(ms, "MultiStartMpc", type("Refuse", (), {"__init__": no_handle}))
    x0, goal = np.array([[-7.0, -7.0, 0.7, 0.0, 0.0]]), [7.0, 7.0]
    assert ms.episode_arguments(x0, goal, "RANDOM")["guess_geometry"] is None
    assert ms.episode_arguments(x0, goal, "RANDOM", guess_geometry=True)["guess_geometry"] == gc.GEOM
    assert ms.sweep_arguments(x0[0], goal, "RANDOM", (0, 4), 2)["guess_geometry"] is None
    assert ms.sweep_arguments(x0[0], goal, "RANDOM", (0, 4), 2, guess_geometry=dict(lead=0.5))["guess_geometry"] == dict(gc.GEOM, lead=0.5)
    for call in (lambda: ms.run_multistart_episodes(x0, goal, "RANDOM", guess_geometry=dict(a_max=0.0)),
                 lambda: ms.run_multistart_sweep(x0[0], goal, "RANDOM", (0, 4), 2, guess_geometry="yes")):
        with pytest.raises(ValueError, match="guess_geometry"):
            call()
