"""Multi-start solves on the GPU (mpc_seed_guesses_dev, mpc_select_best_dev, mpc_gpu.MultiStartMpc):

  1. the guess kernel against the numpy family (multistart_cases.guesses) at 1e-12 -- entries are below 10 in magnitude and the device's sin / cos /
     atan2 are within a few ulp --, keep_first, the L < 1e-9 row bit for bit mpc_reset_guess_dev's, canary rows behind the last instance;
  2. the selection kernel on synthetic tables against the numpy rule (multistart_cases.select), exactly: winner, best_cost, best_u0; with broadcast every
     member's rows bit for bit the winner's, without it X and U untouched, a group without a winner untouched, canaries intact; the refusals;
  3. MultiStartMpc.solve on the parity scenes against the oracle's group solve: every candidate by helpers.judge_against_oracle (one iteration) or by
     the rule test_gpu_sqp.py applies to its launches (four iterations: statuses and iteration counts equal, 1e-6 on X, 8e-6 on U and u0, 1e-8 relative
     on the cost) -- no tolerance of this file's own --, the winners equal, best_u0 bit for bit the winner's u0;
  4. six MultiStartMpc.step calls in lockstep with the oracle: in front of every step the oracle side restarts from the GPU's read-back state and member
     iterates, so the single-step tolerances apply and nothing drifts; winner sequences equal; one case with incumbent_margin = 0.1; a group without
     a winner coasts and is reseeded whole;
  5. per-scenario masks, weights, bounds and set_sqp given to MultiStartMpc against the replicated arrays set on the inner handle, bit for bit.
test_multistart_host.py holds what makes 3 and 4 fair (statuses 0, cost gaps >= 1e-4 on the oracle alone)."""
import ctypes as C

import numpy as np
import pytest

import multistart_cases as mc
from feature_loop import Banded, make, mg, on_own_stream      # noqa: F401 (mg is a fixture)
from helpers import judge_against_oracle

pytestmark = pytest.mark.gpu
CANARY = 2           # rows behind instance G K - 1 that no launch may touch
SENTINEL = -3.5e33


def _dev(torch):
    return torch.device("cuda:0")


def _up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev(torch))


def _lib_call(mpc_gpu, fn, *args):
    return getattr(mpc_gpu._lib.lib(), fn)(*args)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------------------------------------------- 1. the guesses
G_SEED = 3


def _seed_inputs(K):
    x0 = np.array([[-5.0, -5.0, 0.7, 0.4, -0.2], [3.0, -1.0, -4.0, 1.5, 0.3], [1.0, 2.0, 0.3, 0.7, -0.2]])
    goal = np.array([[5.0, 5.0], [-4.5, 2.25], [1.0, 2.0]])          # the second group's heading is more than half a turn from its path: the wrap acts;
                                                                     # the last group stands on its goal: L = 0
    off = {1: np.array([2.5]), 5: np.array(mc.OFFSETS)}.get(K, np.linspace(-6.0, 6.0, K))
    return x0, goal, off


def _seed(mpc_gpu, torch, N, K):
    x0, goal, off = _seed_inputs(K)
    B = G_SEED * K
    q = torch.cuda.current_stream().cuda_stream
    with make(mpc_gpu, N, 3, B) as s:
        bd = Banded(torch, _dev(torch))
        dx0, dg, doff = bd.f64(G_SEED, 5), bd.f64(G_SEED, 2), bd.f64(K)
        dx0.copy_(_up(torch, x0)); dg.copy_(_up(torch, goal)); doff.copy_(_up(torch, off))
        dX, dU = bd.f64(B + CANARY, N + 1, 5, init=SENTINEL), bd.f64(B + CANARY, N, 2, init=SENTINEL)
        torch.cuda.current_stream().synchronize()
        h = s._h
        assert _lib_call(mpc_gpu, "mpc_seed_guesses_dev", h, G_SEED, K, _p(dx0), _p(dg), _p(doff), 0, _p(dX), _p(dU), q) == 0
        torch.cuda.current_stream().synchronize()
        X, U = dX.cpu().numpy().copy(), dU.cpu().numpy().copy()
        # keep_first on arrays that hold something else
        rng = np.random.default_rng(N * 100 + K)
        X1, U1 = rng.uniform(-9, 9, X.shape), rng.uniform(-9, 9, U.shape)
        dX.copy_(_up(torch, X1)); dU.copy_(_up(torch, U1))
        torch.cuda.current_stream().synchronize()
        assert _lib_call(mpc_gpu, "mpc_seed_guesses_dev", h, G_SEED, K, _p(dx0), _p(dg), _p(doff), 1, _p(dX), _p(dU), q) == 0
        torch.cuda.current_stream().synchronize()
        Xk, Uk = dX.cpu().numpy().copy(), dU.cpu().numpy().copy()
        # the plain reset guess of the same states, per instance
        dXr, dUr = bd.f64(B, N + 1, 5, init=SENTINEL), bd.f64(B, N, 2, init=SENTINEL)
        dxr = bd.f64(B, 5); dxr.copy_(_up(torch, np.repeat(x0, K, axis=0)))
        torch.cuda.current_stream().synchronize()
        s.reset_guess_dev(B, dxr, dXr, dUr, stream=q)
        torch.cuda.current_stream().synchronize()
        assert bd.intact()
        assert np.array_equal(dx0.cpu().numpy(), x0) and np.array_equal(dg.cpu().numpy(), goal) and np.array_equal(doff.cpu().numpy(), off)
        return dict(X=X, U=U, Xk=Xk, Uk=Uk, X1=X1, U1=U1, Xr=dXr.cpu().numpy(), Ur=dUr.cpu().numpy())


def _guesses_against_numpy(mg, N, K):
    import torch
    mpc_gpu, _ = mg
    x0, goal, off = _seed_inputs(K)
    B = G_SEED * K
    r = _seed(mpc_gpu, torch, N, K)
    want = [mc.guesses(x0[g], goal[g], off, N) for g in range(G_SEED)]
    Xw, Uw = np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want])
    err = np.abs(r["X"][:B] - Xw).max()
    print(f"MULTISTART-SEED N={N} K={K}: worst |GPU - numpy| over X {err:.3e}")
    assert np.abs(Xw).max() < 10.0
    assert err <= 1e-12
    assert np.array_equal(r["U"][:B], Uw) and not r["U"][:B].any()
    # exact parts: stage 0 is x0, v and omega are zero beyond it
    rows = np.arange(B)[np.arange(B) // K < 2]
    assert np.array_equal(r["X"][rows, 0], np.repeat(x0[:2], K, axis=0)) and not r["X"][:B, 1:, 3:].any()
    # the group on its goal: mpc_reset_guess_dev's rows, bit for bit
    on_goal = np.arange(2 * K, 3 * K)
    assert np.array_equal(r["X"][on_goal], r["Xr"][on_goal]) and np.array_equal(r["U"][on_goal], r["Ur"][on_goal])
    # canaries
    assert (r["X"][B:] == SENTINEL).all() and (r["U"][B:] == SENTINEL).all()
    # keep_first: member 0 of every group bitwise what the arrays held, the others what the plain call wrote, the canary rows what the arrays held
    first = np.arange(G_SEED) * K
    others = np.setdiff1d(np.arange(B), first)
    assert np.array_equal(r["Xk"][first], r["X1"][first]) and np.array_equal(r["Uk"][first], r["U1"][first])
    assert np.array_equal(r["Xk"][others], r["X"][others]) and np.array_equal(r["Uk"][others], r["U"][others])
    assert np.array_equal(r["Xk"][B:], r["X1"][B:]) and np.array_equal(r["Uk"][B:], r["U1"][B:])


@pytest.mark.parametrize("K", [1, 5, 64])
@pytest.mark.parametrize("N", [2, 20, 62])
def test_guesses_against_numpy(mg, N, K):
    on_own_stream(_guesses_against_numpy, mg, N, K)


def _non_finite_inputs_propagate(mg):
    import torch
    mpc_gpu, _ = mg
    N, K = 20, mc.K
    with mpc_gpu.MultiStartMpc(N, mc.NO, 2.0, scenarios=2) as ms:
        x0, goal, obst = (np.stack([a, a]) for a in mc.scene("C"))
        x0[1, 1] = np.nan
        out = ms.solve(x0, obst, goal)
        torch.cuda.synchronize()
        X = ms.iterates()[0].cpu().numpy()
        assert out["cand_status"].cpu().numpy()[1].tolist() == [4] * K and out["winner"].cpu().numpy().tolist()[1] == -1
        assert out["winner"].cpu().numpy()[0] == mc.select(out["cand_cost"].cpu().numpy()[0], out["cand_status"].cpu().numpy()[0])[0] >= 0
        assert np.isnan(X[1, :, :, 1]).all()                       # the NaN went into the iterate (and a status 4 leaves the iterate alone)
        assert np.isinf(out["cost"].cpu().numpy()[1]) and not out["u0"].cpu().numpy()[1].any()


def test_non_finite_inputs_propagate_and_the_group_has_no_winner(mg):
    on_own_stream(_non_finite_inputs_propagate, mg)


# ---------------------------------------------------------------------------------------------------------------- 2. the selection
G_SEL = 7


def _random_table(K, seed):
    """G_SEL groups: random costs and statuses with ties, NaN, infinities and failed members sprinkled in; group 3 has no eligible member, group 5 is
    all ties"""
    rng = np.random.default_rng(seed)
    cost = rng.uniform(1.0, 100.0, (G_SEL, K))
    status = rng.choice(np.array([0, 0, 0, 2, 4], np.int32), (G_SEL, K)).astype(np.int32)
    if K >= 2:
        cost[1, rng.integers(K)] = cost[1].min()                   # a tie with the least member (possibly itself)
        cost[4, rng.integers(K)] = -np.inf
        cost[6, rng.integers(K)] = np.inf
        # group 2: every member converged, the last one of more than two with a NaN cost, member 0 at 1.5 times the least of the others --
        # beaten with margin 0.25 (1 < 0.75 x 1.5), kept with margin 0.6 (1 > 0.4 x 1.5)
        status[2] = 0
        cost[2, 0] = 1.5 * cost[2, 1:K - 1 if K > 2 else K].min()
        if K > 2:
            cost[2, K - 1] = np.nan
    if K == 64:
        cost[0, 47], status[0, 47] = 0.5, 0                        # a winner in the upper half of the wavefront
    status[3] = 4
    cost[5] = 42.0; status[5] = 0
    return cost, status


def _select(mpc_gpu, torch, N, cost, status, margin, flags, with_u0=True):
    """one mpc_select_best_dev on a fresh handle over random iterates; everything read back"""
    G, K = cost.shape
    B = G * K
    q = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(7 * N + K)
    X0, U0 = rng.uniform(-9, 9, (B + CANARY, N + 1, 5)), rng.uniform(-9, 9, (B + CANARY, N, 2))
    u0 = rng.uniform(-8, 8, (B + CANARY, 2))
    with make(mpc_gpu, N, 3, B) as s:
        bd = Banded(torch, _dev(torch))
        dc, ds = bd.f64(B + CANARY), bd.i32(B + CANARY)
        dc[:B].copy_(_up(torch, cost.reshape(-1))); ds[:B].copy_(_up(torch, status.reshape(-1)))
        dX, dU, du0 = bd.f64(*X0.shape), bd.f64(*U0.shape), bd.f64(*u0.shape)
        dX.copy_(_up(torch, X0)); dU.copy_(_up(torch, U0)); du0.copy_(_up(torch, u0))
        dw, dbc, dbu = bd.i32(G + CANARY, init=-77), bd.f64(G + CANARY, init=SENTINEL), bd.f64(G + CANARY, 2, init=SENTINEL)
        torch.cuda.current_stream().synchronize()
        rc = _lib_call(mpc_gpu, "mpc_select_best_dev", s._h, G, K, _p(dc), _p(ds), float(margin), int(flags), _p(dX), _p(dU), _p(dw), _p(dbc), _p(dbu),
                       _p(du0) if with_u0 else None, q)
        assert rc == 0, mpc_gpu._lib.lib().mpc_last_error()
        torch.cuda.current_stream().synchronize()
        g = lambda t: t.cpu().numpy().copy()
        return dict(X0=X0, U0=U0, u0=u0, X=g(dX), U=g(dU), winner=g(dw), best_cost=g(dbc), best_u0=g(dbu), intact=bd.intact(),
                    inputs_kept=np.array_equal(g(dc)[:B], cost.reshape(-1), equal_nan=True) and np.array_equal(g(ds)[:B], status.reshape(-1))
                    and np.array_equal(g(du0), u0))


def _check_selection(r, cost, status, margin, broadcast, with_u0=True):
    G, K = cost.shape
    B = G * K
    N = r["X0"].shape[1] - 1
    src_u0 = r["u0"][:B].reshape(G, K, 2) if with_u0 else r["U0"][:B, 0].reshape(G, K, 2)
    w, c, b = mc.select_groups(cost, status, margin, src_u0)
    assert r["intact"] and r["inputs_kept"]
    assert np.array_equal(r["winner"][:G], w), (r["winner"][:G], w)
    assert np.array_equal(r["best_cost"][:G], c) and np.array_equal(r["best_u0"][:G], b)
    assert (r["winner"][G:] == -77).all() and (r["best_cost"][G:] == SENTINEL).all() and (r["best_u0"][G:] == SENTINEL).all()
    Xw, Uw = r["X0"].copy(), r["U0"].copy()
    if broadcast:
        for g in range(G):
            if w[g] >= 0:
                Xw[g * K:(g + 1) * K] = r["X0"][g * K + w[g]]; Uw[g * K:(g + 1) * K] = r["U0"][g * K + w[g]]
    assert np.array_equal(r["X"], Xw) and np.array_equal(r["U"], Uw)      # (the canary rows and every group without a winner included)
    return w


def _selection_on_random_tables(mg, N, K):
    import torch
    mpc_gpu, _ = mg
    SB = mpc_gpu._lib.SELECT_BROADCAST
    cost, status = _random_table(K, seed=1000 * N + K)
    seen = []
    for margin, flags, with_u0 in ((0.0, SB, True), (0.0, 0, True), (0.25, SB, False), (0.6, 0, True)):
        r = _select(mpc_gpu, torch, N, cost, status, margin, flags, with_u0)
        seen.append(_check_selection(r, cost, status, margin, bool(flags & SB), with_u0).tolist())
    print(f"MULTISTART-SELECT N={N} K={K}: winners {seen[0]}, with margin 0.25 {seen[2]}, with margin 0.6 {seen[3]}")
    assert seen[0] == seen[1] and seen[0][3] == -1 and seen[0][5] == 0
    if K >= 2:       # the margin decides group 2: beaten at 0.25, kept at 0.6
        assert seen[0][2] == seen[2][2] > 0 and seen[3][2] == 0
    if K == 64:      # the tables reach both halves of the wavefront
        assert seen[0][0] == 47 and min(w for w in seen[0] if w >= 0) < 32


@pytest.mark.parametrize("K", [1, 2, 5, 64])
@pytest.mark.parametrize("N", [2, 31, 62])
def test_selection_on_random_tables(mg, N, K):
    assert (5 * (N + 1)) % 64 and (2 * N) % 64      # row lengths that are no multiple of the wavefront
    on_own_stream(_selection_on_random_tables, mg, N, K)


def _selection_on_hand_made_tables(mg, K):
    import torch
    mpc_gpu, _ = mg
    SB = mpc_gpu._lib.SELECT_BROADCAST
    for margin, cost, status in mc.hand_table(K):
        for flags in (SB, 0):
            w = _check_selection(_select(mpc_gpu, torch, 31, cost, status, margin, flags), cost, status, margin, bool(flags))
        if K == 5:
            assert w.tolist() == [h[4] for h in mc.HAND if h[3] == margin]


@pytest.mark.parametrize("K", [1, 2, 5, 64])
def test_selection_on_the_hand_made_tables_of_the_host_test(mg, K):
    on_own_stream(_selection_on_hand_made_tables, mg, K)


def _refusals(mg):
    import torch
    mpc_gpu, _ = mg
    L, ERR = mpc_gpu._lib.lib(), mpc_gpu._lib.MPC_ERR_ARG
    q = torch.cuda.current_stream().cuda_stream
    N, G, K = 5, 2, 5
    with make(mpc_gpu, N, 3, G * K) as s:
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=_dev(torch))
        x0, goal, off, X, U, cost, u0 = z(G, 5), z(G, 2), z(K), z(G * K, N + 1, 5), z(G * K, N, 2), z(G * K), z(G * K, 2)
        status, win = torch.zeros(G * K, dtype=torch.int32, device=_dev(torch)), torch.full((G,), -77, dtype=torch.int32, device=_dev(torch))
        torch.cuda.current_stream().synchronize()
        seed = lambda g=G, k=K, a=x0, b=goal, c=off, d=X, e=U: L.mpc_seed_guesses_dev(s._h, g, k, _p(a), _p(b), _p(c), 0, _p(d), _p(e), q)
        sel = lambda g=G, k=K, c=cost, st=status, m=0.0, f=0, x=X, u=U, w=win, bu=None, uu=None: \
            L.mpc_select_best_dev(s._h, g, k, _p(c), _p(st), m, f, _p(x), _p(u), _p(w), None, _p(bu), _p(uu), q)
        for call, word in ((lambda: seed(k=0), b"K must be"), (lambda: seed(k=65), b"K must be"), (lambda: seed(g=3), b"max_batch"), (lambda: seed(g=-1), b"max_batch"),
                           (lambda: seed(a=None), b"null"), (lambda: seed(b=None), b"null"), (lambda: seed(c=None), b"null"), (lambda: seed(d=None), b"null"),
                           (lambda: seed(e=None), b"null"),
                           (lambda: sel(k=0), b"K must be"), (lambda: sel(k=65), b"K must be"), (lambda: sel(g=3), b"max_batch"),
                           (lambda: sel(c=None), b"null"), (lambda: sel(st=None), b"null"), (lambda: sel(w=None), b"null"),
                           (lambda: sel(m=-0.01), b"incumbent_margin"), (lambda: sel(m=1.0), b"incumbent_margin"), (lambda: sel(m=float("nan")), b"incumbent_margin"),
                           (lambda: sel(f=2), b"flags"), (lambda: sel(f=1, x=None), b"MPC_SELECT_BROADCAST"), (lambda: sel(f=1, u=None), b"MPC_SELECT_BROADCAST"),
                           (lambda: sel(u=None, bu=u0), b"d_best_u0")):
            assert call() == ERR and word in L.mpc_last_error(), (word, L.mpc_last_error())
        # what is allowed: no groups; the optional outputs absent; X and U absent without the broadcast
        assert seed(g=0) == 0 and sel(g=0) == 0 and sel() == 0 and sel(x=None, u=None) == 0 and sel(m=0.999, f=1) == 0
        torch.cuda.current_stream().synchronize()
        assert win.cpu().numpy().tolist() == [0, 0]          # (all costs 0 and eligible: ties go to member 0)


def test_refusals_and_optional_arguments(mg):
    on_own_stream(_refusals, mg)


# ---------------------------------------------------------------------------------------------------------------- 3. against the oracle on the parity scenes
def _launches():
    out = {}
    for name, N, Tf, it in mc.PARITY:
        out.setdefault((N, Tf, it), []).append(name)
    return out


LAUNCHES = _launches()      # one MultiStartMpc.solve per (N, Tf, iterations): its scenes are the groups


def _judge_candidates(orc, cfg, o, x, g, Xg, Ug, it, tag):
    """the K candidates of ONE group: GPU (g: dict of u0, cost, status, iters, sqp_iters; iterates Xg, Ug) against the oracle's group solve o"""
    Kk = len(o["cost"])
    x0, goal, P = np.tile(x, (Kk, 1)), np.tile(o["goal"], (Kk, 1)), np.tile(o["P"], (Kk, 1, 1, 1))
    if it == 1:
        n = judge_against_oracle(orc, cfg, x0, P, goal, o["X0"], o["U0"], g, Xg, Ug, o)
        assert n["converged"] == Kk and n["status_borderline"] == 0, n
        print(f"{tag}: {n}")
    else:      # test_gpu_sqp.py's rule for a launch of several iterations
        dX, dU = np.abs(Xg - o["X"]).max(axis=(1, 2)), np.abs(Ug - o["U"]).max(axis=(1, 2))
        du0 = np.abs(g["u0"] - o["u0"]).max(axis=1)
        print(f"{tag}: worst |dX| {dX.max():.3e} |dU| {dU.max():.3e} |du0| {du0.max():.3e}; interior-point iterations {g['iters'].tolist()} vs {o['iters'].tolist()}")
        assert np.array_equal(g["status"], o["status"]), (g["status"], o["status"])
        assert np.array_equal(g["sqp_iters"], o["sqp_iters"]), (g["sqp_iters"], o["sqp_iters"])
        assert (dX <= 1e-6).all(), dX
        assert (dU <= 8e-6).all() and (du0 <= 8e-6).all(), (dU, du0)
        assert np.allclose(g["cost"], o["cost"], rtol=1e-8, atol=1e-8)


def _parity(mg, key):
    import torch
    mpc_gpu, orc = mg
    N, Tf, it = key
    names = LAUNCHES[key]
    G, K = len(names), mc.K
    os_ = [mc.oracle_group(orc, n, N, Tf, it) for n in names]
    x0, goal, obst = (np.stack([o[k] for o in os_]) for k in ("x0", "goal", "obst"))
    with mpc_gpu.MultiStartMpc(N, mc.NO, Tf, scenarios=G, offsets=mc.OFFSETS) as ms:
        ms.inner.set_instance_scheduling(False)
        nsqp = torch.full((G * K,), -77, dtype=torch.int32, device=_dev(torch))
        if it > 1:
            ms.set_sqp(it, 0.0)
            ms.inner.set_sqp_iters_out(nsqp)
        out = ms.solve(x0, obst, goal, keep_solution=True)
        torch.cuda.synchronize()
        c = lambda t: t.cpu().numpy().copy()
        cand = dict(u0=c(out["cand_u0"]), cost=c(out["cand_cost"]), status=c(out["cand_status"]), iters=c(out["cand_iters"]), sqp_iters=c(nsqp).reshape(G, K))
        Xs, Us = c(ms.solved_X).reshape(G, K, N + 1, 5), c(ms.solved_U).reshape(G, K, N, 2)
        Xb, Ub = (c(t) for t in ms.iterates())
        winner, cost, u0 = c(out["winner"]), c(out["cost"]), c(out["u0"])
    for g, (name, o) in enumerate(zip(names, os_)):
        tag = f"MULTISTART-PARITY {name} N={N} iterations={it}"
        _judge_candidates(orc, o["cfg"], o, o["x0"], {k: v[g] for k, v in cand.items()}, Xs[g], Us[g], it, tag)
        w = int(winner[g])
        print(f"{tag}: winner {w} (oracle {o['winner']}), cost {cost[g]:.6g} against member 0's {cand['cost'][g, 0]:.6g}")
        assert w == o["winner"] == mc.select(cand["cost"][g], cand["status"][g])[0]
        assert cost[g] == cand["cost"][g, w] and np.array_equal(u0[g], cand["u0"][g, w])          # bit for bit the winner's
        assert np.array_equal(u0[g], Us[g, w, 0])                                                  # ... which is U[0] of its iterate
        for k in range(K):                                                                         # behind the broadcast every member holds the winner
            assert np.array_equal(Xb[g, k], Xs[g, w]) and np.array_equal(Ub[g, k], Us[g, w])


@pytest.mark.parametrize("key", list(LAUNCHES), ids=[f"N{N}-it{it}" for N, Tf, it in LAUNCHES])
def test_group_solve_against_the_oracle_on_the_parity_scenes(mg, key):
    on_own_stream(_parity, mg, key)


# ---------------------------------------------------------------------------------------------------------------- 4. the closed loop in lockstep
def _lockstep(mg, name, margin):
    import torch
    mpc_gpu, orc = mg
    N, Tf, K = mc.LOCKSTEP_N, mc.LOCKSTEP_TF, mc.K
    x0, goal, obst0 = mc.scene(name)
    cfg = orc.config(N, mc.NO, Tf)
    c = lambda t: t.cpu().numpy().copy()
    winners, oracle_winners = [], []
    with mpc_gpu.MultiStartMpc(N, mc.NO, Tf, scenarios=1, offsets=mc.OFFSETS, incumbent_margin=margin) as ms:
        ms.inner.set_instance_scheduling(False)
        x, obst, dgoal = _up(torch, x0[None]), _up(torch, obst0[None]), _up(torch, goal[None])
        for k in range(mc.LOCKSTEP_STEPS):
            torch.cuda.synchronize()
            xa, oa = c(x)[0], c(obst)[0]                                   # the state this step starts from, read back
            if k == 0:
                Xa, Ua = mc.guesses(xa, goal, mc.OFFSETS, N)               # (the first step seeds every member itself: test 1 holds the kernel to these)
            else:
                Xa, Ua = (c(t)[0] for t in ms.iterates())
            out = ms.step(x, obst, dgoal, keep_solution=True)
            torch.cuda.synchronize()
            o, xo, oo, Xo, Uo = mc.oracle_step(orc, cfg, xa, oa, goal, Xa, Ua, margin)
            o["goal"] = goal
            g = dict(u0=c(out["cand_u0"])[0], cost=c(out["cand_cost"])[0], status=c(out["cand_status"])[0], iters=c(out["cand_iters"])[0])
            Xs, Us = c(ms.solved_X).reshape(K, N + 1, 5), c(ms.solved_U).reshape(K, N, 2)
            _judge_candidates(orc, cfg, o, xa, g, Xs, Us, 1, f"MULTISTART-LOCKSTEP {name} margin {margin} step {k}")
            w = int(c(out["winner"])[0])
            winners.append(w); oracle_winners.append(o["winner"])
            assert w == o["winner"] == mc.select(g["cost"], g["status"], margin)[0] and w >= 0
            assert np.array_equal(c(out["u0"])[0], g["u0"][w])
            # behind the step: plant and obstacles moved, member 0 on the winner's shifted iterate (bit for bit: a shift copies), the others reseeded
            xb, ob = c(x)[0], c(obst)[0]
            Xb, Ub = (c(t)[0] for t in ms.iterates())
            assert np.abs(xb - orc.dynamics(xa, g["u0"][w], Tf / N)[0]).max() <= 1e-12      # (the plant step with the GPU's own u0: test_gpu_aux.py sees 1e-13)
            assert np.abs(ob - oo).max() <= 1e-12
            Xsh, Ush = orc.shift(cfg, Xs[w], Us[w])
            assert np.array_equal(Xb[0], Xsh) and np.array_equal(Ub[0], Ush)
            Xg, Ug = mc.guesses(xb, goal, mc.OFFSETS, N)
            assert np.abs(Xb[1:] - Xg[1:]).max() <= 1e-12 and not Ub[1:].any()
    print(f"MULTISTART-LOCKSTEP {name} margin {margin}: winners {winners} (oracle {oracle_winners})")
    assert winners == oracle_winners
    assert winners == [r["winner"] for r in mc.oracle_loop(orc, name, margin)]      # ... and the sequence the oracle takes when it drives itself


@pytest.mark.parametrize("case", mc.LOCKSTEP, ids=mc.LOCKSTEP_IDS)
def test_closed_loop_in_lockstep_with_the_oracle(mg, case):
    on_own_stream(_lockstep, mg, *case)


def _a_group_without_a_winner(mg):
    """two scenarios, the second with a NaN obstacle: every member of it fails (status 4), it applies u = 0, and the step reseeds it whole"""
    import torch
    mpc_gpu, orc = mg
    N, Tf, K = mc.LOCKSTEP_N, mc.LOCKSTEP_TF, mc.K
    x0, goal, obst0 = mc.scene("C")
    c = lambda t: t.cpu().numpy().copy()
    with mpc_gpu.MultiStartMpc(N, mc.NO, Tf, scenarios=2) as ms:
        x, dgoal = _up(torch, np.stack([x0, x0])), _up(torch, np.stack([goal, goal]))
        ob = np.stack([obst0, obst0]); ob[1, 1, 0] = np.nan
        obst = _up(torch, ob)
        for k in range(2):
            xa = c(x)
            out = ms.step(x, obst, dgoal)
            torch.cuda.synchronize()
            assert c(out["winner"])[1] == -1 and c(out["winner"])[0] >= 0 and c(out["cand_status"])[1].tolist() == [4] * K
            assert np.isinf(c(out["cost"])[1]) and not c(out["u0"])[1].any()
            xb = c(x)
            assert np.abs(xb[1] - orc.dynamics(xa[1], np.zeros(2), Tf / N)[0]).max() <= 1e-12         # u = 0: it coasts
            Xb, Ub = (c(t) for t in ms.iterates())
            Xg, Ug = mc.guesses(xb[1], goal, mc.OFFSETS, N)
            assert np.abs(Xb[1] - Xg).max() <= 1e-12 and not Ub[1].any()                              # all K members, member 0 included
            assert np.abs(Xb[0, 0] - mc.guesses(xb[0], goal, mc.OFFSETS, N)[0][0]).max() > 1e-3       # the live group keeps its shifted winner


def test_a_group_without_a_winner_coasts_and_is_reseeded_whole(mg):
    on_own_stream(_a_group_without_a_winner, mg)


# ---------------------------------------------------------------------------------------------------------------- 5. the pass-through of the per-instance features
def _pass_through(mg):
    """per-SCENARIO rows given to MultiStartMpc reach the inner handle replicated per group: the same solve as with the replicated per-instance arrays set
    on the inner handle directly, bit for bit, and the two scenarios (one scene, different rows) do differ"""
    import torch
    mpc_gpu, _ = mg
    K = mc.K
    x0, goal, obst = (np.stack([a, a]) for a in mc.scene("B"))
    active = np.array([[True, True, True], [False, True, True]])                 # scenario 1 does not see the obstacle on the line
    W = np.array([[2.0, 2.0, 2.0, 2.0, 0.15, 0.15], [3.0, 3.0, 1.0, 1.0, 0.3, 0.3]])
    bu_hi = np.array([[8.0, 8.0], [4.0, 6.0]])
    c = lambda t: t.cpu().numpy().copy()
    res = []
    for direct in (False, True):
        with mpc_gpu.MultiStartMpc(20, mc.NO, 2.0, scenarios=2) as ms:
            ms.inner.set_instance_scheduling(False)
            if direct:
                ms.inner.set_obstacle_mask(np.repeat(active, K, axis=0))
                ms.inner.set_instance_params(W=np.repeat(W, K, axis=0))
                ms.inner.set_instance_bounds(bu_hi=np.repeat(bu_hi, K, axis=0))
                ms.inner.set_sqp(2, 0.0)
            else:
                ms.set_obstacle_mask(active)
                ms.set_instance_params(W=W)
                ms.set_instance_bounds(bu_hi=bu_hi)
                ms.set_sqp(2, 0.0)
            out = ms.solve(x0, obst, goal)
            torch.cuda.synchronize()
            res.append({k: c(v) for k, v in out.items()})
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k]), k
    assert (res[0]["cand_status"] != 4).all() and (res[0]["winner"] >= 0).all()
    assert not np.array_equal(res[0]["cand_cost"][0], res[0]["cand_cost"][1])


def test_per_scenario_features_reach_the_inner_handle_replicated(mg):
    on_own_stream(_pass_through, mg)
