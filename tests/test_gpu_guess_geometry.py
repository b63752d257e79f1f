"""The guess family from geometry on the GPU (mpc_set_guess_geometry, mpc_seed_guesses_geom_dev, the GEOM instantiations of the group control step and of
the group refill, MultiStartMpc(guess_geometry=...)).  The yardstick is the numpy restatement of the rule (guess_geometry_cases.amplitudes) with the numpy
guess family (multistart_cases.guesses), and the kernels that existed before; never the new kernels themselves.  Tolerance 1e-12 as test_gpu_multistart.py
holds the family to: entries are below 10 in magnitude, and the device's sin / atan2 are within a few ulp.

  1. mpc_seed_guesses_geom_dev against numpy at (N, K, n_obst) = (2, 1, 1), (20, 5, 3), (20, 8, 3), (62, 5, 10), (20, 5, 32): 7 groups of the hand-made scenes
     and the random table of 64 groups, keep_first, canary rows, the amplitudes in offsets_out; the tie-and-clamp scene bit for bit in offsets_out;
  2. groups without a blocking obstacle equal mpc_seed_guesses_dev bit for bit;
  3. the obstacle mask, a per-instance r_safe row that turns a blocker into a non-blocker, a NaN obstacle (it does not block; the other groups are untouched);
  4. mode on and off again: group step (two steps) and group refill bit-identical to a handle that never had it on;
  5. the group step with the mode on in lockstep over 6 steps on scenes C and the moved B: member 0 the shifted winner, the reseeded members the rule on the
     GPU's own new state and moved obstacles; a group without a winner; an idle group;
  6. the group refill with the mode on: a started group's members against the rule on its read-back start row and drawn obstacles; kept, parked and drained
     groups as before;
  7. MultiStartMpc: step against step_fused, 4 steps; run_multistart_sweep (6 seeds, 3 slots) against run_multistart_episodes on 6 groups;
  8. the refusals.
test_guess_geometry_host.py holds what makes the comparisons fair (decision gaps >= 1e-6 on numpy and the oracle alone)."""
import ctypes as C

import numpy as np
import pytest

import guess_geometry_cases as gc
import multistart_cases as mc
import multistart_sweep_cases as sc
from feature_loop import Banded, make, mg, on_own_stream      # noqa: F401 (mg is a fixture)
from test_gpu_multistart_episodes import Rig as StepRig
from test_gpu_multistart_sweep import Rig as RefillRig, _progress, sc_rows

pytestmark = pytest.mark.gpu
CANARY = 2
SENTINEL = -3.5e33
TOL = 1e-12


def _dev(torch):
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _geom_on(mpc_gpu, s, geom):
    L = mpc_gpu._lib.lib()
    assert L.mpc_set_guess_geometry(s._h, 1, geom["clearance"], geom["a_max"], geom["lead"]) == 0, L.mpc_last_error()


def _geom_off(mpc_gpu, s):
    assert mpc_gpu._lib.lib().mpc_set_guess_geometry(s._h, 0, 0.0, 1.0, 0.0) == 0


def _seed_geom(mpc_gpu, torch, s, K, x, obst, goal, off, keep_first=0, fill=None, plain=False):
    """one launch on guard-banded arrays with canary rows: X, U (G K + CANARY rows) and offsets_out (G + CANARY rows) as numpy arrays; fill: what X and U
    hold before the launch ((X, U) numpy arrays) instead of the sentinel; plain: mpc_seed_guesses_dev on the same inputs instead"""
    G, N, no = x.shape[0], s.N, s.n_obst
    B = G * K
    q = torch.cuda.current_stream().cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(_dev(torch))
    bd = Banded(torch, _dev(torch))
    dx, do, dg, doff = bd.f64(G, 5), bd.f64(G, no, 4), bd.f64(G, 2), bd.f64(K)
    dx.copy_(up(x)); do.copy_(up(obst)); dg.copy_(up(goal)); doff.copy_(up(off))
    dX, dU, dout = bd.f64(B + CANARY, N + 1, 5, init=SENTINEL), bd.f64(B + CANARY, N, 2, init=SENTINEL), bd.f64(G + CANARY, K, init=SENTINEL)
    if fill is not None:
        dX.copy_(up(fill[0])); dU.copy_(up(fill[1]))
    torch.cuda.current_stream().synchronize()
    L = mpc_gpu._lib.lib()
    if plain:
        rc = L.mpc_seed_guesses_dev(s._h, G, K, _p(dx), _p(dg), _p(doff), keep_first, _p(dX), _p(dU), q)
    else:
        rc = L.mpc_seed_guesses_geom_dev(s._h, G, K, _p(dx), _p(do), _p(dg), _p(doff), keep_first, _p(dX), _p(dU), _p(dout), q)
    assert rc == 0, L.mpc_last_error()
    torch.cuda.current_stream().synchronize()
    assert bd.intact()
    for t, a in ((dx, x), (do, obst), (dg, goal), (doff, off)):
        assert np.array_equal(t.cpu().numpy(), np.asarray(a, dtype=np.float64), equal_nan=True)      # the inputs are inputs
    return dX.cpu().numpy(), dU.cpu().numpy(), dout.cpu().numpy()


def _against_numpy(tag, X, U, out, x, goal, obst, off, geom, N, r=None, active=None):
    """one launch's arrays against the rule and the family in numpy; returns the amplitudes (G, K)"""
    G, K = x.shape[0], len(off)
    B = G * K
    amps, gaps, nb = gc.group_amplitudes(x, goal, obst, off, geom, r, active)
    Xw, Uw = gc.group_guesses(x, goal, amps, N)
    ea, ex = np.abs(out[:G] - amps).max(), np.abs(X[:B] - Xw).max()
    print(f"GUESS-GEOMETRY {tag}: blockers {nb.min()} .. {nb.max()}, least gap {gaps.min():.3g}; worst |GPU - numpy| amplitudes {ea:.3e} X {ex:.3e}")
    assert np.abs(Xw).max() < 16.0                                # (positions within 6 of the origin, amplitudes clamped to 6: the tolerance is some hundred ulp)
    assert ea <= TOL and ex <= TOL
    assert np.array_equal(out[:G, 0], np.full(G, off[0])) and not U[:B].any()
    assert (X[B:] == SENTINEL).all() and (U[B:] == SENTINEL).all() and (out[G:] == SENTINEL).all()
    return amps


# ---------------------------------------------------------------------------------------------------------------- 1. the seed launch against numpy
SHAPES = [(2, 1, 1), (20, 5, 3), (20, 8, 3), (62, 5, 10), (20, 5, 32)]
G_HAND = 7           # not a multiple of the four instances per workgroup, nor is 7 K for K = 1, 5


def _offsets(K):
    return {1: np.array([0.0]), 5: np.array(mc.OFFSETS)}.get(K, np.linspace(-3.5, 3.5, K))


def _seed_against_numpy(mg, N, K, no):
    import torch
    mpc_gpu, _ = mg
    off = _offsets(K)
    with make(mpc_gpu, N, no, gc.RANDOM_G * K) as s:
        for lead in (0.0, 1.0):
            geom = dict(gc.GEOM, lead=lead)
            _geom_on(mpc_gpu, s, geom)
            x, goal, obst = gc.hand_table(G_HAND, no, lead)
            X, U, out = _seed_geom(mpc_gpu, torch, s, K, x, obst, goal, off)
            _against_numpy(f"hand N={N} K={K} no={no} lead={lead}", X, U, out, x, goal, obst, off, geom, N)
            if lead == 0.0:                                       # keep_first on arrays that hold something else
                rng = np.random.default_rng(N + K)
                X1, U1 = rng.uniform(-9, 9, X.shape), rng.uniform(-9, 9, U.shape)
                Xk, Uk, outk = _seed_geom(mpc_gpu, torch, s, K, x, obst, goal, off, keep_first=1, fill=(X1, U1))
                first = np.arange(G_HAND) * K
                others = np.setdiff1d(np.arange(G_HAND * K), first)
                assert np.array_equal(Xk[first], X1[first]) and np.array_equal(Uk[first], U1[first])
                assert np.array_equal(Xk[others], X[others]) and np.array_equal(Uk[others], U[others])
                assert np.array_equal(Xk[G_HAND * K:], X1[G_HAND * K:]) and np.array_equal(outk, out)      # offsets_out: member 0 included
        geom = dict(gc.GEOM, lead=gc.RANDOM_LEAD)
        _geom_on(mpc_gpu, s, geom)
        x, goal, obst = gc.random_table(no)
        X, U, out = _seed_geom(mpc_gpu, torch, s, K, x, obst, goal, off)
        amps = _against_numpy(f"random N={N} K={K} no={no}", X, U, out, x, goal, obst, off, geom, N)
        if K > 1:
            assert (amps != off).any()


@pytest.mark.parametrize("shape", SHAPES, ids=["N%d-K%d-no%d" % s for s in SHAPES])
def test_the_seed_launch_against_numpy(mg, shape):
    on_own_stream(_seed_against_numpy, mg, *shape)


def _tie_and_clamp(mg):
    import torch
    mpc_gpu, _ = mg
    t = gc.TIE
    x, goal, obst, off = np.array([t["x0"]]), np.array([t["goal"]]), np.array([t["obst"]]), np.array(t["offsets"])
    with make(mpc_gpu, 20, 3, len(off)) as s:
        _geom_on(mpc_gpu, s, gc.HAND)
        X, U, out = _seed_geom(mpc_gpu, torch, s, len(off), x, obst, goal, off)
        print(f"GUESS-GEOMETRY tie and clamp: amplitudes {out[0].tolist()}")
        assert out[0].tolist() == list(t["want"])                 # bit for bit: the clamp, the tie to the lower index, the base fallback
        Xw, _ = mc.guesses(x[0], goal[0], np.array(t["want"]), 20)
        assert np.abs(X[:len(off)] - Xw).max() <= TOL
        # scene A by hand: (0, 2.7, -2.3, 5, -5)
        x0, gl, ob = mc.scene("A")
        X, U, out = _seed_geom(mpc_gpu, torch, s, mc.K, x0[None], ob[None], gl[None], np.array(mc.OFFSETS))
        assert np.abs(out[0] - np.array(gc.SCENE_A_WANT)).max() <= 1e-15 and out[0, 3:].tolist() == [5.0, -5.0]


def test_the_tie_and_clamp_scene_bit_for_bit(mg):
    on_own_stream(_tie_and_clamp, mg)


# ---------------------------------------------------------------------------------------------------------------- 2. no blocker: the fixed family, bit for bit
def _no_blocker(mg):
    import torch
    mpc_gpu, _ = mg
    N, no, K = 20, 3, mc.K
    off = np.array(mc.OFFSETS)
    x, goal, obst = gc.hand_table(6, no, 0.0)
    obst[1, :, :2] += 30.0                                        # group 1: every obstacle far off the line
    obst[4, :, 0] -= 40.0                                         # group 4: every obstacle behind the robot (s < 0)
    x[5, :2] = goal[5]                                            # group 5 stands on its goal (L = 0): the base family, which then writes the plain guess
    with make(mpc_gpu, N, no, 6 * K) as s:
        _geom_on(mpc_gpu, s, gc.GEOM)
        X, U, out = _seed_geom(mpc_gpu, torch, s, K, x, obst, goal, off)
        Xp, Up, _ = _seed_geom(mpc_gpu, torch, s, K, x, obst, goal, off, plain=True)
        amps, gaps, nb = gc.group_amplitudes(x, goal, obst, off, gc.GEOM)
        assert nb.tolist()[1] == 0 and nb.tolist()[4] == 0 and nb[[0, 2, 3]].min() >= 1
        for g in (1, 4, 5):
            rows = slice(g * K, (g + 1) * K)
            assert np.array_equal(X[rows], Xp[rows]) and np.array_equal(U[rows], Up[rows]) and out[g].tolist() == off.tolist()
        for g in (0, 2, 3):                                       # member 0, and members beyond the candidates, keep the base offset: the same bits too
            keep = [k for k in range(K) if amps[g, k] == off[k]]
            assert 0 in keep
            for k in keep:
                assert np.array_equal(X[g * K + k], Xp[g * K + k])
            assert not np.array_equal(X[g * K + 1], Xp[g * K + 1])


def test_groups_without_a_blocker_get_the_fixed_family_bit_for_bit(mg):
    on_own_stream(_no_blocker, mg)


# ---------------------------------------------------------------------------------------------------------------- 3. mask, radii, NaN
def _mask_radii_nan(mg):
    import torch
    mpc_gpu, _ = mg
    N, no, K, G = 20, 3, mc.K, 4
    off = np.array(mc.OFFSETS)
    x, goal, obst = (np.stack([a] * G) for a in gc.scene("C"))    # two blockers: obstacles 0 and 1
    with make(mpc_gpu, N, no, G * K) as s:
        _geom_on(mpc_gpu, s, gc.GEOM)
        base = _seed_geom(mpc_gpu, torch, s, K, x, obst, goal, off)
        # the mask of row g K: group 1 does not see obstacle 0, group 2 sees nothing
        active = np.ones((G, no), bool); active[1, 0] = False; active[2] = False
        s.set_obstacle_mask(np.repeat(active, K, axis=0))
        X, U, out = _seed_geom(mpc_gpu, torch, s, K, x, obst, goal, off)
        amps = _against_numpy("mask", X, U, out, x, goal, obst, off, gc.GEOM, N, active=active)
        assert out[2].tolist() == off.tolist() and np.array_equal(out[0], base[2][0]) and not np.array_equal(out[1], base[2][1])
        s.set_obstacle_mask(None)
        # per-instance r_safe: in group 3 obstacle 0 shrinks to 0.01 -- |c| is above 0.26 there -- and no longer blocks; group 1's obstacle 1 grows
        r = np.full((G, no), gc.R_SAFE); r[3, 0] = 0.01; r[1, 1] = 3.1
        s.set_instance_params(r_safe=np.repeat(r, K, axis=0))
        X, U, out = _seed_geom(mpc_gpu, torch, s, K, x, obst, goal, off)
        amps = _against_numpy("r_safe rows", X, U, out, x, goal, obst, off, gc.GEOM, N, r=r)
        nb = gc.group_amplitudes(x, goal, obst, off, gc.GEOM, r)[2]
        assert nb.tolist() == [2, 2, 2, 1] and np.array_equal(out[0], base[2][0]) and np.array_equal(out[2], base[2][2])      # (an untouched row: the same bits)
        s.set_instance_params()
        # a NaN obstacle does not block; the other groups' words are those of the launch without it
        ob = obst.copy(); ob[1, 0] = np.nan
        X, U, out = _seed_geom(mpc_gpu, torch, s, K, x, ob, goal, off)
        _against_numpy("NaN obstacle", X, U, out, x, goal, ob, off, gc.GEOM, N)
        assert np.isfinite(X[:G * K]).all() and not np.array_equal(out[1], base[2][1])
        for g in (0, 2, 3):
            assert np.array_equal(X[g * K:(g + 1) * K], base[0][g * K:(g + 1) * K]) and np.array_equal(out[g], base[2][g])


def test_mask_radii_and_a_nan_obstacle(mg):
    on_own_stream(_mask_radii_nan, mg)


# ---------------------------------------------------------------------------------------------------------------- 4. on and off again: the bits of a handle that never had it on
def _step_twice(mpc_gpu, torch, toggle):
    N, no, K, G = 20, 3, mc.K, 2
    x0, goal, obst = gc.hand_table(G, no, 0.0)
    with make(mpc_gpu, N, no, G * K) as s:
        if toggle:
            _geom_on(mpc_gpu, s, gc.GEOM); _geom_off(mpc_gpu, s)
        rig = StepRig(mpc_gpu, torch, s, G, K, mc.OFFSETS, goal)
        rig.load(x0, obst)
        snaps = []
        for _ in range(2):
            rig.solve()
            assert rig.tail(0.0) == 0
            snaps.append(rig.snapshot())
    return snaps


def _refill_once(mpc_gpu, torch, toggle):
    N, no, K, G, count = 8, 5, 3, 3, 4
    start, goal_rows = sc_rows(count, np.random.default_rng(11))
    with make(mpc_gpu, N, no, count * K) as s:
        if toggle:
            _geom_on(mpc_gpu, s, gc.GEOM); _geom_off(mpc_gpu, s)
        rig = RefillRig(mpc_gpu, torch, s, G, K, count, (0.0, 2.5, -2.5), start, goal_rows)
        assert rig.call() == 0
        return rig.snapshot()


def _on_and_off(mg):
    import torch
    mpc_gpu, _ = mg
    a, b = _step_twice(mpc_gpu, torch, False), _step_twice(mpc_gpu, torch, True)
    for sa, sb in zip(a, b):
        for n in sa:
            assert np.array_equal(sa[n], sb[n], equal_nan=True), n
    assert (a[1]["winner"][:2] >= 0).all()
    ra, rb = _refill_once(mpc_gpu, torch, False), _refill_once(mpc_gpu, torch, True)
    for n in ra:
        assert np.array_equal(ra[n], rb[n], equal_nan=True), n
    assert (ra["slot_seed"] >= 0).all()


def test_on_and_off_again_gives_the_bits_of_a_handle_that_never_had_it_on(mg):
    on_own_stream(_on_and_off, mg)


# ---------------------------------------------------------------------------------------------------------------- 5. the group step, mode on
def _step_lockstep(mg, name, margin):
    import torch
    mpc_gpu, orc = mg
    N, Tf, K, no = mc.LOCKSTEP_N, mc.LOCKSTEP_TF, mc.K, mc.NO
    x0, goal, obst0 = gc.scene(name)
    cfg = orc.config(N, no, Tf)
    off = np.array(mc.OFFSETS)
    winners, worst = [], 0.0
    with make(mpc_gpu, N, no, K) as s:
        _geom_on(mpc_gpu, s, gc.GEOM)
        rig = StepRig(mpc_gpu, torch, s, 1, K, mc.OFFSETS, goal[None])
        rig.load(x0[None], obst0[None], seed=False)
        assert rig.L.mpc_seed_guesses_geom_dev(s._h, 1, K, _p(rig.x), _p(rig.obst), _p(rig.goal), _p(rig.off), 0, _p(rig.X), _p(rig.U), None, rig.q) == 0
        for k in range(mc.LOCKSTEP_STEPS):
            rig.solve()
            pre = rig.snapshot()
            assert rig.tail(margin) == 0, rig.L.mpc_last_error()
            post = rig.snapshot()
            assert rig.bd.intact()
            w = int(post["winner"][0])
            winners.append(w)
            assert w == mc.select(pre["key"][:K], pre["status"][:K], margin)[0] and w >= 0
            Xsh, Ush = orc.shift(cfg, pre["X"][w], pre["U"][w])
            assert np.array_equal(post["X"][0], Xsh) and np.array_equal(post["U"][0], Ush)      # member 0: the winner's shifted iterate (a shift copies)
            xb, ob = post["x"][0], post["obst"][0]                                                # the GPU's own new state and moved obstacles
            amps, info = gc.amplitudes(xb, goal, ob, off, **gc.GEOM)
            assert info["gap"] >= 1e-6
            Xg, _ = mc.guesses(xb, goal, amps, N)
            d = np.abs(post["X"][1:K] - Xg[1:]).max()
            worst = max(worst, d)
            assert d <= TOL and not post["U"][1:K].any(), (k, d)
            assert not np.array_equal(amps, off)
            for n in ("X", "U", "mx", "mobst"):                                                   # canary rows
                assert np.array_equal(post[n][K:], pre[n][K:]), n
    want = [r["winner"] for r in gc.oracle_loop(orc, name, margin)[1:]]
    print(f"GUESS-GEOMETRY lockstep {name} margin {margin}: winners {winners} (oracle alone {want}); worst |reseeded - numpy| {worst:.3e}")
    assert winners == want


@pytest.mark.parametrize("case", gc.LOCKSTEP, ids=gc.LOCKSTEP_IDS)
def test_the_group_step_in_lockstep_with_the_rule(mg, case):
    on_own_stream(_step_lockstep, mg, *case)


def _step_lost_and_idle(mg):
    """three groups of scene C: group 0 runs, group 1 has no eligible member (every status 4) and is reseeded whole, member 0 with offsets[0]; group 2 is idle"""
    import torch
    mpc_gpu, _ = mg
    N, no, K, G = 20, 3, mc.K, 3
    off = np.array(mc.OFFSETS)
    x0, goal, obst = gc.hand_table(G, no, 1.0)
    geom = dict(gc.GEOM, lead=1.0)
    with make(mpc_gpu, N, no, G * K) as s:
        _geom_on(mpc_gpu, s, geom)
        rig = StepRig(mpc_gpu, torch, s, G, K, mc.OFFSETS, goal)
        rig.load(x0, obst)
        rig.solve()
        rig.status[K:2 * K] = 4
        rig.flags[2] = 1
        pre = rig.snapshot()
        assert rig.tail(0.0) == 0
        post = rig.snapshot()
        assert rig.bd.intact() and post["winner"][:2].tolist()[1] == -1 and post["winner"][0] >= 0 and post["lost"][:G].tolist() == [0, 1, 0]
        amps, info = gc.amplitudes(post["x"][1], goal[1], post["obst"][1], off, **geom)
        Xg, _ = mc.guesses(post["x"][1], goal[1], amps, N)
        assert info["gap"] >= 1e-6 and amps[0] == 0.0 and not np.array_equal(amps, off)
        assert np.abs(post["X"][K:2 * K] - Xg).max() <= TOL and not post["U"][K:2 * K].any()      # all K members, member 0 included
        for n in list(rig.F64) + list(rig.I32):                   # the idle group: none of its words
            rows = slice(2 * K, None) if dict(rig.F64, **rig.I32)[n][0] else slice(2, None)
            assert np.array_equal(post[n][rows], pre[n][rows], equal_nan=True), n


def test_the_group_step_with_a_lost_and_an_idle_group(mg):
    on_own_stream(_step_lost_and_idle, mg)


# ---------------------------------------------------------------------------------------------------------------- 6. the group refill, mode on
def _refill(mg):
    import torch
    mpc_gpu, _ = mg
    from mpc_gpu import world
    N, no, K, G = 20, 5, 5, 5
    roles = ["flag", "keep", "budget", "keep", "flag"]
    count = G + 2                                                 # three finish, two seeds are left: the last finished group is drained
    rng = np.random.default_rng(77)
    start, goal_rows = sc_rows(count, rng)
    off = np.array(mc.OFFSETS)
    geom = dict(gc.GEOM, lead=0.5)
    worst, acted = 0.0, 0

    def started_rows(post, assign):
        nonlocal worst, acted
        for g in np.nonzero(np.asarray(assign) >= 0)[0]:
            rows = slice(g * K, (g + 1) * K)
            amps, info = gc.amplitudes(post["x"][g], post["goal"][g], post["obst"][g], off, **geom)      # the read-back start row and drawn obstacles
            assert info["gap"] >= 1e-6, (g, info)
            Xg, _ = mc.guesses(post["x"][g], post["goal"][g], amps, N)
            d = np.abs(post["X"][rows] - Xg).max()
            worst, acted = max(worst, d), acted + int(not np.array_equal(amps, off))
            assert d <= TOL and not post["U"][rows].any(), (g, d)
            assert np.array_equal(post["x"][g], start[assign[g]]) and np.array_equal(post["goal"][g], goal_rows[assign[g]])

    with make(mpc_gpu, N, no, count * K) as s:
        _geom_on(mpc_gpu, s, geom)
        rig = RefillRig(mpc_gpu, torch, s, G, K, count, mc.OFFSETS, start, goal_rows)
        pre = rig.snapshot()
        want, assign = rig.model(world, pre)
        assert rig.call() == 0, rig.L.mpc_last_error()
        post = rig.snapshot()
        assert rig.bd.intact() and assign.tolist() == list(range(G))
        for n in sc.ARRAYS:
            if n != "X":
                assert np.array_equal(post[n], want[n], equal_nan=True), n
        started_rows(post, assign)
        # kept, parked and started, parked and drained
        pre = _progress(post, roles, rng)
        rig.put(pre)
        want, assign = rig.model(world, pre)
        assert rig.call() == 0
        post = rig.snapshot()
        assert rig.bd.intact() and assign.tolist() == [G, sc.KEEP, G + 1, sc.KEEP, sc.DRAIN]
        for n in sc.ARRAYS:
            if n != "X":
                assert np.array_equal(post[n], want[n], equal_nan=True), n
        not_started = np.repeat(np.asarray(assign) < 0, K)
        assert np.array_equal(post["X"][not_started], pre["X"][not_started])                         # kept and drained groups: not a word of their iterates
        started_rows(post, assign)
    print(f"GUESS-GEOMETRY refill: worst |seeded - numpy| {worst:.3e}; the rule acted on {acted} of 7 started groups")
    assert acted >= 1


def test_the_group_refill_with_the_rule(mg):
    on_own_stream(_refill, mg)


# ---------------------------------------------------------------------------------------------------------------- 7. the drivers
def _step_against_step_fused(mg):
    import torch
    mpc_gpu, _ = mg
    N, no, K, G = 20, 3, mc.K, 2
    x0, goal, obst = (np.stack([gc.scene(n)[i] for n in ("C", "Bm")]) for i in (0, 1, 2))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev(torch))
    c = lambda t: t.cpu().numpy().copy()
    runs = []
    for fused in (False, True):
        with mpc_gpu.MultiStartMpc(N, no, 2.0, scenarios=G, offsets=mc.OFFSETS, guess_geometry=True) as ms:
            ms.inner.set_instance_scheduling(False)
            x, ob, gl = up(x0), up(obst), up(goal)
            rec = []
            for k in range(4):
                out = (ms.step_fused if fused else ms.step)(x, ob, gl)
                torch.cuda.synchronize()
                rec.append(dict(winner=c(out["winner"]), u0=c(out["u0"]), x=c(x), obst=c(ob), X=c(ms.X), U=c(ms.U)))
            first = c(ms.member_offsets)
            runs.append((rec, first))
    amps0 = gc.group_amplitudes(x0, goal, obst, np.array(mc.OFFSETS), gc.GEOM)[0]
    assert np.abs(runs[1][1] - amps0).max() <= TOL                # step_fused's one stand-alone seed launch: the first
    worst = 0.0
    for a, b in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(a["winner"], b["winner"]) and (a["winner"] >= 0).all()
        worst = max([worst] + [np.abs(a[n] - b[n]).max() for n in ("u0", "x", "obst", "X", "U")])
    print(f"GUESS-GEOMETRY step against step_fused: winners {[r['winner'].tolist() for r in runs[0][0]]}; worst difference {worst:.3e}")
    assert worst <= 1e-9                                          # (the bound the fused driver is held to against the composed loop)
    last = runs[0][0][-1]
    amps = gc.group_amplitudes(last["x"], goal, last["obst"], np.array(mc.OFFSETS), gc.GEOM)[0]
    assert np.abs(runs[0][1] - amps).max() <= TOL                 # step's last reseed wrote member_offsets
    assert not np.array_equal(amps, np.tile(mc.OFFSETS, (G, 1)))


def test_step_against_step_fused(mg):
    on_own_stream(_step_against_step_fused, mg)


def _sweep_against_batch(mg):
    mpc_gpu, _ = mg
    start, goal = [-7.0, -7.0, np.pi / 4, 0.0, 0.0], [7.0, 7.0]
    kw = dict(incumbent_margin=0.1, N=20, Tf=2.0, n_obst=5, max_iter=8, guess_geometry=dict(lead=0.5))
    ref = mpc_gpu.run_multistart_episodes(np.tile(start, (6, 1)), goal, "RANDOM", first_seed=40, **kw)
    r = mpc_gpu.run_multistart_sweep(start, goal, "RANDOM", (40, 6), 3, poll_every=1, **kw)
    close = lambda a, b: float(np.abs(np.where(a == b, 0.0, a - b)).max())
    print(f"GUESS-GEOMETRY sweep: switched {r['switched_steps'].tolist()} lost {r['lost_steps'].tolist()}; largest |sweep - batch| table "
          f"{close(r['table'], ref['table']):.3e} x_last {close(r['x_last'], ref['x_last']):.3e}")
    assert np.array_equal(r["table"][:, [0, 1, 4, 5]], ref["table"][:, [0, 1, 4, 5]])
    assert np.array_equal(r["lost_steps"], ref["lost_steps"]) and np.array_equal(r["switched_steps"], ref["switched_steps"])
    assert close(r["table"], ref["table"]) <= 1e-9 and close(r["x_last"], ref["x_last"]) <= 1e-9
    assert r["steps_run"] == 16 and r["solves"] == ref["solves"] == 5 * 6 * 8


def test_the_sweep_against_the_batch(mg):
    on_own_stream(_sweep_against_batch, mg)


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def _refusals(mg):
    import torch
    mpc_gpu, _ = mg
    ERR = mpc_gpu._lib.MPC_ERR_ARG
    L = mpc_gpu._lib.lib()
    N, no, K, G = 5, 2, 3, 2
    nan, inf = float("nan"), float("inf")
    with make(mpc_gpu, N, no, G * K) as s:
        f64 = lambda *sh: torch.full(sh, SENTINEL, dtype=torch.float64, device=_dev(torch))
        x, ob, gl, off, X, U, out = f64(G, 5), f64(G, no, 4), f64(G, 2), f64(K), f64(G * K, N + 1, 5), f64(G * K, N, 2), f64(G, K)
        q = torch.cuda.current_stream().cuda_stream
        args = dict(h=s._h, G=G, K=K, x=_p(x), ob=_p(ob), gl=_p(gl), off=_p(off), X=_p(X), U=_p(U), out=_p(out))
        call = lambda **kw: (lambda a: L.mpc_seed_guesses_geom_dev(a["h"], a["G"], a["K"], a["x"], a["ob"], a["gl"], a["off"], 0, a["X"], a["U"], a["out"], q))(dict(args, **kw))
        assert call() == ERR and b"guess geometry is off" in L.mpc_last_error()                     # the mode is off on a new handle
        for bad in ((2, 0.25, 6.0, 0.0), (-1, 0.25, 6.0, 0.0), (1, -0.1, 6.0, 0.0), (1, nan, 6.0, 0.0), (1, inf, 6.0, 0.0), (1, 0.25, 0.0, 0.0), (1, 0.25, -6.0, 0.0),
                    (1, 0.25, nan, 0.0), (1, 0.25, inf, 0.0), (1, 0.25, 6.0, -0.5), (1, 0.25, 6.0, nan), (1, 0.25, 6.0, inf)):
            assert L.mpc_set_guess_geometry(s._h, *bad) == ERR and b"mpc_set_guess_geometry" in L.mpc_last_error(), bad
        assert call() == ERR                                      # a refused setting leaves the mode off
        _geom_on(mpc_gpu, s, gc.GEOM)
        for kw, word in ((dict(h=None), b"null handle"), (dict(K=0), b"K must be"), (dict(K=65), b"K must be"), (dict(G=-1), b"max_batch"), (dict(G=3), b"max_batch")) \
                + tuple((({n: None}), b"null device pointer") for n in ("x", "ob", "gl", "off", "X", "U")):
            assert call(**kw) == ERR and word in L.mpc_last_error(), (kw, L.mpc_last_error())
        s.set_obstacle_mask(np.ones((G * K - 1, no), bool))       # a mask that covers fewer instances than groups * K
        assert call() == ERR and b"covers fewer" in L.mpc_last_error()
        s.set_obstacle_mask(None)
        torch.cuda.synchronize()
        assert all(bool((t == SENTINEL).all()) for t in (X, U, out))                                 # nothing was launched
        assert call(G=0) == 0 and call(out=None) == 0             # no group: nothing to do; offsets_out may be null
        _geom_off(mpc_gpu, s)
        assert call() == ERR and b"guess geometry is off" in L.mpc_last_error()
    with pytest.raises(ValueError, match="guess_geometry"):
        mpc_gpu.MultiStartMpc(N, no, 0.5, scenarios=1, guess_geometry=dict(a_max=-1.0))
    with mpc_gpu.MultiStartMpc(N, no, 0.5, scenarios=2, offsets=(0.0, 1.0)) as ms:
        assert ms.guess_geometry is None and ms.member_offsets is None
        with pytest.raises(ValueError, match="guess_geometry"):
            mpc_gpu.run_multistart_episodes(np.zeros((2, 5)), [5.0, 5.0], np.zeros((2, no, 4)), offsets=(0.0, 1.0), solver=ms, guess_geometry=True)


def test_refusals(mg):
    on_own_stream(_refusals, mg)
