"""The rollout merit on the GPU (mpc_rollout_merit_dev, BatchedMpc.rollout_merit_dev, MultiStartMpc(select_by="rollout")):

  1. every output against the checker's (rollout_merit_cases: X^r by chaining oracle.dynamics, merit = oracle.cost at (X^r, U), defect / margin / boxviol in
     numpy) on random finite U within the bounds and X = X^r + 1e-2 noise -- X^r, defect, margin, boxviol at 1e-10 absolute, merit at 1e-8 relative
     (the module's docstring says where the two bounds come from) -- over N in {2, 20, 31, 62}, 1 / 3 / 10 obstacles and 32 at N = 31, batch 1 and 5 with
     members = 1 and batch 9 with members = 3; guard bands and canary rows intact, inputs untouched; a second launch gives identical bits; an output that is
     not asked for is not written; a NaN in one instance's U gives a non-finite merit there and leaves the neighbours bit-identical;
  2. one case per feature (explicit slack schedule with a hole, per-stage reference with offsets, per-instance W / We / r_safe / r_hit, obstacle mask,
     per-instance bounds): with the feature set the figures are the checker's with it, without it the checker's without, and the two differ by > 1e-4;
  3. the refusals that need a handle;
  4. MultiStartMpc(select_by="rollout"): cand_merit / cand_defect / cand_margin against the checker on the members' solved iterates as read back, the winners
     the numpy rule on the oracle's own merits (every scene, one with margin 0.1), `cost` the winner's merit; four step() calls in lockstep with the oracle,
     restarted from the GPU's read-back state as test_gpu_multistart.py does;
  5. select_by="cost" against a MultiStartMpc built without the argument: every result tensor and every iterate bit for bit, and no new field.
test_rollout_merit_host.py holds what makes these comparisons sharp."""
import numpy as np
import pytest

import multistart_cases as mc
import rollout_merit_cases as rc
from feature_loop import Banded, make, mg, on_own_stream      # noqa: F401 (mg is a fixture)
from helpers import judge_against_oracle

pytestmark = pytest.mark.gpu
CANARY = 2           # rows behind the last instance that no launch may touch
SENTINEL = -3.5e33
OUTPUTS = ("merit", "defect", "margin", "boxviol", "Xr")


def _dev(torch):
    return torch.device("cuda:0")


def _up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev(torch))


class _Call:
    """the device arrays of one case on one handle: inputs uploaded once, guard-banded; `run` launches and reads the outputs asked for back"""

    def __init__(self, torch, s, c, B, N, no):
        self.torch, self.s, self.B, self.N, self.members = torch, s, B, N, c["members"]
        bd = self.bd = Banded(torch, _dev(torch))
        self.src = dict(x0=c["x0"], P=c["P"], goal=c["goal"], U=c["U"], X=c["X"])
        self.inp = {}
        for k, a in self.src.items():
            self.inp[k] = bd.f64(*a.shape); self.inp[k].copy_(_up(torch, a))
        self.out = dict(merit=bd.f64(B + CANARY, init=SENTINEL), defect=bd.f64(B + CANARY, init=SENTINEL), margin=bd.f64(B + CANARY, init=SENTINEL),
                        boxviol=bd.f64(B + CANARY, init=SENTINEL), Xr=bd.f64(B + CANARY, N + 1, 5, init=SENTINEL))
        torch.cuda.current_stream().synchronize()

    def set_U(self, U):
        self.src["U"] = U
        self.inp["U"].copy_(_up(self.torch, U))

    def run(self, want=OUTPUTS, with_X=True):
        torch = self.torch
        for t in self.out.values():
            t.fill_(SENTINEL)
        torch.cuda.current_stream().synchronize()
        i = self.inp
        self.s.rollout_merit_dev(self.B, i["x0"], i["P"], i["goal"], i["U"], X=i["X"] if with_X else None, members=self.members,
                                 stream=torch.cuda.current_stream().cuda_stream, **{k: self.out[k] for k in want})
        torch.cuda.current_stream().synchronize()
        r = {k: t.cpu().numpy().copy() for k, t in self.out.items()}
        assert self.bd.intact()
        for k, a in self.src.items():                            # the inputs are inputs
            assert np.array_equal(self.inp[k].cpu().numpy(), a, equal_nan=True), k
        for k, a in r.items():                                   # canary rows, and every output that was not asked for
            assert (a[self.B:] == SENTINEL).all(), k
            if k not in want:
                assert (a == SENTINEL).all(), k
        return {k: a[:self.B] for k, a in r.items()}


def _against_checker(tag, r, want, B):
    """the GPU's figures r against the checker's `want` (dicts of merit, defect, margin, boxviol and, where given, Xr)"""
    err = {k: float(np.abs(r[k] - want[k]).max()) for k in ("defect", "margin", "boxviol", "Xr") if k in want and np.isfinite(want[k]).all()}
    rel = float(rc.rel_change(r["merit"], want["merit"]).max())
    print(f"{tag}: worst |GPU - checker| {({k: '%.2e' % v for k, v in err.items()})}, merit relative {rel:.2e}")
    for k, v in err.items():
        assert v <= rc.TOL_ABS, (k, v)
    for k in ("margin",):                                        # (an infinite margin is compared exactly)
        if k in want:
            assert np.array_equal(np.isinf(r[k]), np.isinf(want[k])) and np.array_equal(r[k][np.isinf(want[k])], want[k][np.isinf(want[k])])
    assert rel <= rc.TOL_MERIT, (r["merit"], want["merit"])


# ---------------------------------------------------------------------------------------------------------------- 1. parity on the random cases
def _parity(mg, shp):
    import torch
    mpc_gpu, orc = mg
    N, no, B, m = shp
    c = rc.case(orc, *shp)
    with make(mpc_gpu, N, no, B) as s:
        call = _Call(torch, s, c, B, N, no)
        r = call.run()
        _against_checker(f"ROLLOUT-PARITY N={N} n_obst={no} batch={B} members={m}", r, c, B)
        # the same launch again: the same bits
        r2 = call.run()
        for k in OUTPUTS:
            assert np.array_equal(r[k], r2[k]), k
        # every output alone: the others are not written (run checks that), the one asked for has the bits of the full call; the defect alone needs X,
        # the others do without
        for k in OUTPUTS:
            assert np.array_equal(call.run(want=(k,), with_X=(k == "defect"))[k], r[k]), k
        # a NaN in one instance's U: its merit is not finite, the neighbours' figures keep their bits
        bad = B // 2
        U = c["U"].copy()
        U[bad, N // 2, 1] = np.nan
        call.set_U(U)
        r3 = call.run()
        assert not np.isfinite(r3["merit"][bad])
        assert np.isnan(r3["Xr"][bad, N // 2 + 1:, 2]).all() and np.array_equal(r3["Xr"][bad, :N // 2 + 1], r["Xr"][bad, :N // 2 + 1])
        others = np.arange(B) != bad
        for k in OUTPUTS:
            assert np.array_equal(r3[k][others], r[k][others]), k


@pytest.mark.parametrize("shp", rc.SHAPES, ids=rc.SHAPE_IDS)
def test_every_output_against_the_oracle(mg, shp):
    on_own_stream(_parity, mg, shp)


# ---------------------------------------------------------------------------------------------------------------- 2. the features
def _feature(mg, name):
    import torch
    mpc_gpu, orc = mg
    N, no, B, m = rc.FEATURE_SHAPE
    base, f = rc.case(orc, N, no, B, m), rc.feature(orc, name)
    with make(mpc_gpu, N, no, B) as s:
        call = _Call(torch, s, base, B, N, no)
        r0 = call.run()
        _against_checker(f"ROLLOUT-FEATURE {name}, feature off", r0, base, B)
        getattr(s, f["setter"])(**f["set"])
        r1 = call.run()
        want = dict(base, merit=f["merit"], margin=f["margin"], boxviol=f["boxviol"])
        _against_checker(f"ROLLOUT-FEATURE {name}, feature on ({'oracle' if f['by_oracle'] else 'numpy restatement'})", r1, want, B)
        moved = {"alpha": ("merit",), "reference": ("merit",), "params": ("merit", "margin"), "mask": ("merit", "margin"), "bounds": ("boxviol",)}[name]
        for k in ("merit", "margin", "boxviol"):
            ch = rc.rel_change(r1[k], r0[k])
            print(f"ROLLOUT-FEATURE {name}: relative change of {k} on the GPU {ch.tolist()}")
            if k in moved:
                assert ch.max() > rc.MIN_EFFECT, (name, k)
            else:
                assert np.array_equal(r1[k], r0[k]), (name, k)
        assert np.array_equal(r1["Xr"], r0["Xr"]) and np.array_equal(r1["defect"], r0["defect"])      # no feature reaches the plant


@pytest.mark.parametrize("name", rc.FEATURES)
def test_a_feature_set_on_the_handle_reaches_the_figures(mg, name):
    on_own_stream(_feature, mg, name)


def _empty_mask(mg):
    """an instance without any obstacle: the margin is +inf and the merit is the LS cost alone (the numpy restatement; the oracle has no such problem)"""
    import torch
    mpc_gpu, orc = mg
    N, no, B, m = rc.FEATURE_SHAPE
    c = rc.case(orc, N, no, B, m)
    active = np.ones((B, no), bool); active[1] = False
    with make(mpc_gpu, N, no, B) as s:
        call = _Call(torch, s, c, B, N, no)
        s.set_obstacle_mask(active)
        r = call.run()
    want = dict(c, merit=c["merit"].copy(), margin=c["margin"].copy())
    want["merit"][1] = rc.merit_np(c["cfg"], c["x0"][1], c["P"][1], c["goal"][1], c["Xr"][1], c["U"][1], present=active[1])
    want["margin"][1] = np.inf
    _against_checker("ROLLOUT-FEATURE empty mask", r, want, B)
    assert r["margin"][1] == np.inf


def test_an_instance_without_obstacles_has_an_infinite_margin(mg):
    on_own_stream(_empty_mask, mg)


# ---------------------------------------------------------------------------------------------------------------- 3. the refusals
def _refusals(mg):
    import torch
    mpc_gpu, orc = mg
    N, no, B = 5, 3, 4
    L, q = mpc_gpu._lib.lib(), torch.cuda.current_stream().cuda_stream
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=_dev(torch))
    with make(mpc_gpu, N, no, B) as s:
        x0, P, goal, X, U, out = z(B, 5), z(B, N + 1, no, 2), z(B, 2), z(B, N + 1, 5), z(B, N, 2), z(B)
        torch.cuda.current_stream().synchronize()
        call = lambda **kw: s.rollout_merit_dev(**{**dict(batch=B, x0=x0, P=P, goal=goal, U=U, X=X, merit=out, stream=q), **kw})
        for kw, word in ((dict(batch=B + 1), "batch"), (dict(batch=0), "batch"), (dict(members=0), "members"), (dict(merit=None), "no output"),
                         (dict(X=None, defect=out), "d_defect needs d_X"), (dict(U=None), "null device pointer"), (dict(P=None), "null device pointer")):
            with pytest.raises(mpc_gpu.MpcError, match=word):
                call(**kw)
        call(); call(X=None); call(members=B); call(members=B + 3); call(merit=None, Xr=X)      # what is allowed
        s.set_slack_schedule(np.ones((B - 1, N + 1)))                                           # a feature that covers fewer instances than the call
        with pytest.raises(mpc_gpu.MpcError, match="slack schedule"):
            call()
        call(batch=B - 1)
        torch.cuda.current_stream().synchronize()


def test_refusals_and_optional_arguments(mg):
    on_own_stream(_refusals, mg)


# ---------------------------------------------------------------------------------------------------------------- 4. multi-start by rollout merit
def _checker_on_the_read_back_iterates(orc, cfg, x0, P, goal, Xs, Us):
    dt = cfg.Tf / cfg.N
    Xr = [rc.rollout(orc, x0, U, dt) for U in Us]
    return dict(merit=np.array([orc.cost(cfg, x0, P, goal, Xr[k], Us[k]) for k in range(len(Us))]),
                defect=np.array([rc.defect(orc, x0, Xs[k], Us[k], dt) for k in range(len(Us))]),
                margin=np.array([rc.margin(Xr[k], P) for k in range(len(Us))]))


def _judge_group(tag, orc, o, cand, Xs, Us, winner, cost, u0, margin):
    """one group of a select_by="rollout" solve: the candidates' solves as test_gpu_multistart.py judges them, the rollout figures against the checker on the
    iterates as read back, the winner against the numpy rule on the ORACLE's merits"""
    Kk = len(o["cost"])
    n = judge_against_oracle(orc, o["cfg"], np.tile(o["x0"], (Kk, 1)), np.tile(o["P"], (Kk, 1, 1, 1)), np.tile(o["goal"], (Kk, 1)), o["X0"], o["U0"], cand, Xs, Us, o)
    assert n["converged"] == Kk and n["status_borderline"] == 0, n
    want = _checker_on_the_read_back_iterates(orc, o["cfg"], o["x0"], o["P"], o["goal"], Xs, Us)
    got = dict(merit=cand["merit"], defect=cand["defect"], margin=cand["margin_"], boxviol=np.zeros(Kk))
    _against_checker(tag, got, dict(want, boxviol=np.zeros(Kk)), Kk)
    w = int(winner)
    print(f"{tag}: winner {w} (oracle by merit {o['winner']}, by cost {o['winner_by_cost']}), merit {cost:.6g}")
    assert w == o["winner"] == mc.select(cand["merit"], cand["status"], margin)[0] and w >= 0
    assert cost == cand["merit"][w] and np.array_equal(u0, cand["u0"][w]) and np.array_equal(u0, Us[w, 0])      # bit for bit the winner's


def _cand(out, c, g):
    return dict(u0=c(out["cand_u0"])[g], cost=c(out["cand_cost"])[g], status=c(out["cand_status"])[g], iters=c(out["cand_iters"])[g],
                merit=c(out["cand_merit"])[g], defect=c(out["cand_defect"])[g], margin_=c(out["cand_margin"])[g])


def _ms_parity(mg, names, margin):
    import torch
    mpc_gpu, orc = mg
    N, Tf, K, G = rc.MS_N, rc.MS_TF, mc.K, len(names)
    os_ = [rc.ms_group(orc, n, margin) for n in names]
    x0, goal, obst = (np.stack([o[k] for o in os_]) for k in ("x0", "goal", "obst"))
    c = lambda t: t.cpu().numpy().copy()
    with mpc_gpu.MultiStartMpc(N, mc.NO, Tf, scenarios=G, offsets=mc.OFFSETS, incumbent_margin=margin, select_by="rollout") as ms:
        ms.inner.set_instance_scheduling(False)
        out = ms.solve(x0, obst, goal, keep_solution=True)
        torch.cuda.synchronize()
        assert out["cand_merit"].shape == out["cand_defect"].shape == out["cand_margin"].shape == (G, K)
        Xs, Us = c(ms.solved_X).reshape(G, K, N + 1, 5), c(ms.solved_U).reshape(G, K, N, 2)
        Xb, Ub = (c(t) for t in ms.iterates())
        winner, cost, u0 = c(out["winner"]), c(out["cost"]), c(out["u0"])
        cands = [_cand(out, c, g) for g in range(G)]
    differ = 0
    for g, (name, o) in enumerate(zip(names, os_)):
        o = dict(o, goal=o["goal"])
        _judge_group(f"ROLLOUT-MULTISTART {name} margin {margin}", orc, o, cands[g], Xs[g], Us[g], winner[g], cost[g], u0[g], margin)
        differ += int(mc.select(cands[g]["cost"], cands[g]["status"], margin)[0] != int(winner[g]))
        for k in range(K):                                       # behind the broadcast every member holds the winner
            assert np.array_equal(Xb[g, k], Xs[g, int(winner[g])]) and np.array_equal(Ub[g, k], Us[g, int(winner[g])])
    return differ


def _ms_all_scenes(mg):
    differ = _ms_parity(mg, list(rc.MS_SCENES), 0.0)
    assert differ >= 1      # somewhere the reported costs would have picked another member


def test_group_solve_selected_by_rollout_merit(mg):
    on_own_stream(_ms_all_scenes, mg)


def test_group_solve_selected_by_rollout_merit_with_a_margin(mg):
    name, margin = rc.MS_MARGIN_SCENE
    assert margin == 0.1
    on_own_stream(_ms_parity, mg, [name], margin)


def _lockstep(mg, name, margin):
    import torch
    mpc_gpu, orc = mg
    N, Tf, K = rc.MS_N, rc.MS_TF, mc.K
    x0, goal, obst0 = rc.ms_scene(name)
    cfg = orc.config(N, mc.NO, Tf)
    c = lambda t: t.cpu().numpy().copy()
    winners, oracle_winners = [], []
    with mpc_gpu.MultiStartMpc(N, mc.NO, Tf, scenarios=1, offsets=mc.OFFSETS, incumbent_margin=margin, select_by="rollout") as ms:
        ms.inner.set_instance_scheduling(False)
        x, obst, dgoal = _up(torch, x0[None]), _up(torch, obst0[None]), _up(torch, goal[None])
        for k in range(rc.MS_STEPS):
            torch.cuda.synchronize()
            xa, oa = c(x)[0], c(obst)[0]                         # the state this step starts from, read back
            Xa, Ua = mc.guesses(xa, goal, mc.OFFSETS, N) if k == 0 else tuple(c(t)[0] for t in ms.iterates())
            out = ms.step(x, obst, dgoal, keep_solution=True)
            torch.cuda.synchronize()
            o, xo, oo, Xo, Uo = rc.ms_step(orc, cfg, xa, oa, goal, Xa, Ua, margin)
            o.update(cfg=cfg, x0=xa, goal=goal)
            Xs, Us = c(ms.solved_X).reshape(K, N + 1, 5), c(ms.solved_U).reshape(K, N, 2)
            _judge_group(f"ROLLOUT-LOCKSTEP {name} margin {margin} step {k}", orc, o, _cand(out, c, 0), Xs, Us, c(out["winner"])[0], c(out["cost"])[0],
                         c(out["u0"])[0], margin)
            w = int(c(out["winner"])[0])
            winners.append(w); oracle_winners.append(o["winner"])
            xb, ob = c(x)[0], c(obst)[0]
            Xb, Ub = (c(t)[0] for t in ms.iterates())
            assert np.abs(xb - orc.dynamics(xa, c(out["u0"])[0], Tf / N)[0]).max() <= 1e-12 and np.abs(ob - oo).max() <= 1e-12
            Xsh, Ush = orc.shift(cfg, Xs[w], Us[w])
            assert np.array_equal(Xb[0], Xsh) and np.array_equal(Ub[0], Ush)
    print(f"ROLLOUT-LOCKSTEP {name} margin {margin}: winners {winners} (oracle {oracle_winners})")
    assert winners == oracle_winners == [r["winner"] for r in rc.ms_loop(orc, name, margin)]


@pytest.mark.parametrize("case", rc.MS_LOCKSTEP, ids=rc.MS_LOCKSTEP_IDS)
def test_closed_loop_in_lockstep_with_the_oracle(mg, case):
    on_own_stream(_lockstep, mg, *case)


# ---------------------------------------------------------------------------------------------------------------- 5. the default stays what it was
def _cost_is_the_default(mg):
    import torch
    mpc_gpu, _ = mg
    c = lambda t: t.cpu().numpy().copy()
    names = list(rc.MS_SCENES)
    x0, goal, obst = (np.stack([rc.ms_scene(n)[k] for n in names]) for k in range(3))
    res = []
    for kw in ({}, dict(select_by="cost")):
        with mpc_gpu.MultiStartMpc(rc.MS_N, mc.NO, rc.MS_TF, scenarios=len(names), **kw) as ms:
            ms.inner.set_instance_scheduling(False)
            assert ms.select_by == "cost" and not hasattr(ms, "cand_merit")
            rec = []
            out = ms.solve(x0, obst, goal)
            torch.cuda.synchronize()
            rec.append(dict({k: c(v) for k, v in out.items()}, X=c(ms.iterates()[0]), U=c(ms.iterates()[1])))
            x, ob, dg = _up(torch, x0), _up(torch, obst), _up(torch, goal)
            for _ in range(2):
                out = ms.step(x, ob, dg)
                torch.cuda.synchronize()
                rec.append(dict({k: c(v) for k, v in out.items()}, X=c(ms.iterates()[0]), U=c(ms.iterates()[1]), x=c(x), obst=c(ob)))
            res.append(rec)
    for a, b in zip(*res):
        assert set(a) == set(b) and not {"cand_merit", "cand_defect", "cand_margin"} & set(a)
        for k in a:
            assert np.array_equal(a[k], b[k]), k


def test_select_by_cost_is_the_object_built_without_the_argument(mg):
    on_own_stream(_cost_is_the_default, mg)
