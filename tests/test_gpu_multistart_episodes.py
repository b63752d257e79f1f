"""The group control step and its episode driver on the GPU (mpc_group_step_dev, MultiStartMpc.step_fused, run_multistart_episodes).  The yardstick is the
parent's COMPOSITION -- MultiStartMpc.step's sequence of existing entry points (select with broadcast, plant step, obstacle step, shift, reseed, the second
K = 1 seed for the lost groups) run on copies of the state the solve left -- and the numpy restatement of the bookkeeping; never the new kernel itself.

  1. the tail against the composition in lockstep, six control steps at (N, n_obst, K, G) = (2, 1, 1, 1), (20, 3, 5, 5), (62, 10, 2, 3), (31, 12, 3, 2):
     exact winner, best_key, best_u0, member 0's shifted rows, the replicated member inputs, every flag word and counter; 1e-12 on the new state, the
     obstacle states, the seeded rows and min_margin (bit equality is expected and printed); canary rows behind G and G K untouched;
  2. synthetic tables: a group with every status 4, hysteresis keeping member 0, a NaN key, K = 64;
  3. the bookkeeping against numpy: goal reached, arena left, inside an obstacle's r_hit; a per-instance r_hit table; a mask with and without MARGIN_ALL;
  4. idling: a finished group keeps every word over two further fused steps (solve included), its live neighbour in the same workgroup steps on;
  5. run_multistart_episodes against the Python loop over MultiStartMpc.step, twice (the same bits), and an obstacle-free run that ends early;
  6. the argument errors, nothing launched.
test_multistart_episodes_host.py holds what makes 1 and 5 fair (selection gaps >= 1e-4, no threshold within 1e-6, on the oracle alone)."""
import ctypes as C

import numpy as np
import pytest

import multistart_cases as mc
import multistart_episode_cases as ec
from feature_loop import Banded, make, mg, on_own_stream      # noqa: F401 (mg is a fixture)

pytestmark = pytest.mark.gpu
CANARY = 2
SENTINEL = -3.5e33
TOL = 1e-12          # the project's tolerance for guesses and linearisation outputs (test_gpu_multistart.py)


def _dev(torch):
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Rig:
    """the device arrays of G groups of K members on a BatchedMpc `s`, every one with CANARY rows behind it, and the two paths over them"""
    F64 = dict(x=(0, 5), obst=(0, -1, 4), best_key=(0,), best_u0=(0, 2), min_margin=(0,), mx=(1, 5), mobst=(1, -1, 4), mgoal=(1, 2), X=(1, -2, 5), U=(1, -3, 2),
               key=(1,), u0=(1, 2), scr_m=(1,))
    I32 = dict(winner=(0,), flags=(0,), steps=(0,), lost=(0,), switched=(0,), mflags=(1,), status=(1,), iters=(1,), scr_s=(1,))

    def __init__(self, mpc_gpu, torch, s, G, K, offsets, goal):
        self.mpc_gpu, self.torch, self.s, self.G, self.K, self.B = mpc_gpu, torch, s, G, K, G * K
        self.N, self.no = s.N, s.n_obst
        self.bd = Banded(torch, _dev(torch))
        dims = {-1: self.no, -2: self.N + 1, -3: self.N}
        for names, mk in ((self.F64, self.bd.f64), (self.I32, self.bd.i32)):
            for n, sh in names.items():
                rows = (G, self.B)[sh[0]] + CANARY
                setattr(self, n, mk(rows, *[dims.get(d, d) for d in sh[1:]], init=SENTINEL if mk == self.bd.f64 else -77))
        self.goal, self.off = self.up(np.asarray(goal, dtype=np.float64).reshape(G, 2)), self.up(np.asarray(offsets, dtype=np.float64))
        self.offsets = tuple(offsets)
        self.noise = torch.zeros(G, self.no, 2, dtype=torch.float64, device=_dev(torch))
        self.min_margin[:G] = float("inf"); self.scr_m[:self.B] = float("inf")
        for t, n in ((self.flags, G), (self.steps, G), (self.lost, G), (self.switched, G), (self.mflags, self.B), (self.scr_s, self.B)):
            t[:n] = 0
        self.out = mpc_gpu._lib.GroupStepOut(**{f: self.__dict__[a].data_ptr() for f, a in (
            ("winner", "winner"), ("best_key", "best_key"), ("best_u0", "best_u0"), ("min_margin", "min_margin"), ("ep_flags", "flags"), ("ep_steps", "steps"),
            ("lost", "lost"), ("switched", "switched"), ("member_x", "mx"), ("member_obst", "mobst"), ("member_goal", "mgoal"), ("member_flags", "mflags"))})
        self.q = torch.cuda.current_stream().cuda_stream
        self.L = mpc_gpu._lib.lib()

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(_dev(self.torch))

    def sync(self):
        self.torch.cuda.current_stream().synchronize()

    def load(self, x, obst, seed=True):
        """the groups' states into the group arrays and, replicated, the members'; every member seeded"""
        G, K, B = self.G, self.K, self.B
        self.x[:G] = self.up(x); self.obst[:G] = self.up(obst)
        self.mx[:B] = self.up(np.repeat(x, K, axis=0)); self.mobst[:B] = self.up(np.repeat(obst, K, axis=0))
        self.mgoal[:B] = self.goal.repeat_interleave(K, dim=0)
        if seed:
            assert self.L.mpc_seed_guesses_dev(self.s._h, G, K, _p(self.x), _p(self.goal), _p(self.off), 0, _p(self.X), _p(self.U), self.q) == 0
        self.sync()

    def solve(self):
        """the member solve as the driver launches it: STEP_METRICS alone, on the members' flag words and scratch arrays"""
        self.s.closed_loop_step_dev(self.B, self.mx, self.mobst, self.mgoal, self.X, self.U, self.u0, self.key, self.status, self.iters,
                                    flags=self.mpc_gpu._lib.STEP_METRICS, min_margin=self.scr_m, ep_flags=self.mflags, ep_steps=self.scr_s, stream=self.q)
        self.sync()

    def snapshot(self):
        self.sync()
        return {n: getattr(self, n).cpu().numpy().copy() for n in list(self.F64) + list(self.I32)}

    def tail(self, margin, noise=None, flags=0, **kw):
        a = dict(h=self.s._h, G=self.G, K=self.K, key=self.key, status=self.status, u0=self.u0, x=self.x, obst=self.obst, goal=self.goal, off=self.off,
                 X=self.X, U=self.U, out=self.out)
        a.update(kw)
        if noise is not None:
            self.noise.copy_(self.up(noise))
        rc = self.L.mpc_group_step_dev(a["h"], a["G"], a["K"], _p(a["key"]), _p(a["status"]), _p(a["u0"]), float(margin), int(flags), _p(a["x"]), _p(a["obst"]),
                                       _p(a["goal"]), _p(a["off"]), None if noise is None else _p(self.noise), 0.1, 2.0, _p(a["X"]), _p(a["U"]), a["out"], self.q)
        self.sync()
        return rc

    def composed(self, pre, margin, noise=None):
        """the parent's composition on copies of the state `pre`: what MultiStartMpc.step launches behind its solve.  Returns numpy arrays of G / B rows"""
        torch, s, L, G, K, B, N, q = self.torch, self.s, self.L, self.G, self.K, self.B, self.N, self.q
        f64 = lambda *sh: torch.zeros(*sh, dtype=torch.float64, device=_dev(torch))
        X, U, x, obst = (self.up(pre[n][:r]) for n, r in (("X", B), ("U", B), ("x", G), ("obst", G)))
        key, status, u0 = self.up(pre["key"][:B]), self.up(pre["status"][:B]), self.up(pre["u0"][:B])
        w, bc, bu, xn = torch.zeros(G, dtype=torch.int32, device=_dev(torch)), f64(G), f64(G, 2), f64(G, 5)
        X1, U1 = f64(G, N + 1, 5), f64(G, N, 2)
        self.sync()
        assert L.mpc_select_best_dev(s._h, G, K, _p(key), _p(status), float(margin), 1, _p(X), _p(U), _p(w), _p(bc), _p(bu), _p(u0), q) == 0
        s.plant_step_dev(G, x, bu, xn, stream=q)
        s.obstacle_step_dev(G * self.no, obst, None if noise is None else self.up(noise), 0.1, 2.0, stream=q)
        s.shift_dev(B, X, U, stream=q)
        assert L.mpc_seed_guesses_dev(s._h, G, K, _p(xn), _p(self.goal), _p(self.off), 1, _p(X), _p(U), q) == 0
        assert L.mpc_seed_guesses_dev(s._h, G, 1, _p(xn), _p(self.goal), _p(self.off), 0, _p(X1), _p(U1), q) == 0
        self.sync()
        lost = (w < 0)[:, None, None]
        X0, U0 = X.view(G, K, N + 1, 5)[:, 0], U.view(G, K, N, 2)[:, 0]
        X0.copy_(torch.where(lost, X1, X0)); U0.copy_(torch.where(lost, U1, U0))
        self.sync()
        return {n: t.cpu().numpy() for n, t in dict(winner=w, best_key=bc, best_u0=bu, x=xn, obst=obst, X=X, U=U).items()}


def book_numpy(pre, comp, goal, G, r_hit=None, active=None, margin_all=False, arena=(-8.0, 8.0, -8.0, 8.0)):
    """the bookkeeping of the six points in numpy, on the state the COMPOSITION reached: min_margin, flags, steps, lost, switched (G,) for the running groups"""
    x, ob = comp["x"], comp["obst"]
    no = ob.shape[1]
    rh = np.full((G, no), ec.R_HIT) if r_hit is None else r_hit
    d = np.sqrt((x[:, None, 0] - ob[:, :, 0]) ** 2 + (x[:, None, 1] - ob[:, :, 1]) ** 2) - rh
    if active is not None and not margin_all:
        d = np.where(active, d, np.inf)
    mm = np.minimum(pre["min_margin"][:G], d.min(axis=1))
    fl = pre["flags"][:G].copy()
    fl[(x[:, 0] < arena[0]) | (x[:, 0] > arena[1]) | (x[:, 1] < arena[2]) | (x[:, 1] > arena[3])] |= 2
    fl[mm <= 0.0] |= 4
    reached = np.sqrt((x[:, 0] - goal[:, 0]) ** 2 + (x[:, 1] - goal[:, 1]) ** 2) <= ec.TOL_GOAL
    fl[reached] |= 1
    return dict(min_margin=mm, flags=fl, steps=pre["steps"][:G] + ~reached, lost=pre["lost"][:G] + (comp["winner"] < 0), switched=pre["switched"][:G] + (comp["winner"] > 0))


def compare(rig, pre, post, comp, book):
    """the fused tail's arrays `post` against the composition and the numpy bookkeeping, from the state `pre`.  Returns the largest difference seen among the
    values held to TOL."""
    G, K, B = rig.G, rig.K, rig.B
    assert rig.bd.intact()
    live = (pre["flags"][:G] & 1) == 0
    worst = 0.0
    for n in list(rig.F64) + list(rig.I32):                       # canary rows, and every word of an idle group
        rows = (G, B)[(dict(rig.F64, **rig.I32))[n][0]]
        assert np.array_equal(post[n][rows:], pre[n][rows:], equal_nan=True), f"canary rows of {n}"
        if n in ("key", "status", "u0", "iters", "scr_m", "scr_s"):
            assert np.array_equal(post[n], pre[n], equal_nan=True), f"{n} is an input of the tail"
        elif not live.all():
            idle = np.repeat(~live, K) if rows == B else ~live
            assert np.array_equal(post[n][:rows][idle], pre[n][:rows][idle], equal_nan=True), f"{n} of an idle group"
    for g in np.nonzero(live)[0]:
        w = int(comp["winner"][g])
        # exact: the selection, member 0's shifted rows, the replicated inputs, flag words and counters
        assert post["winner"][g] == w and np.array_equal(post["best_key"][g], comp["best_key"][g]) and np.array_equal(post["best_u0"][g], comp["best_u0"][g])
        if w >= 0:
            assert np.array_equal(post["X"][g * K], comp["X"][g * K]) and np.array_equal(post["U"][g * K], comp["U"][g * K])
        for k in range(K):
            assert np.array_equal(post["mx"][g * K + k], post["x"][g]) and np.array_equal(post["mobst"][g * K + k], post["obst"][g])
            assert np.array_equal(post["mgoal"][g * K + k], rig.goal[g].cpu().numpy()) and post["mflags"][g * K + k] == (post["flags"][g] & 1)
        for n in ("flags", "steps", "lost", "switched"):
            assert post[n][g] == book[n][g], (n, g, post[n][g], book[n][g])
        # computed values
        rows = slice(g * K, (g + 1) * K)
        diffs = [np.abs(post["x"][g] - comp["x"][g]).max(), np.abs(post["obst"][g] - comp["obst"][g]).max(), np.abs(post["X"][rows] - comp["X"][rows]).max(),
                 np.abs(post["U"][rows] - comp["U"][rows]).max()]
        if np.isfinite(book["min_margin"][g]) or np.isfinite(post["min_margin"][g]):
            diffs.append(abs(post["min_margin"][g] - book["min_margin"][g]))
        assert max(diffs) <= TOL, (g, diffs)
        worst = max(worst, max(diffs))
    return worst


# ---------------------------------------------------------------------------------------------------------------- 1. lockstep
def lockstep(mpc_gpu, shape):
    """six control steps of one shape's scenes; returns the largest difference seen between the fused tail and the composition"""
    import torch
    N, no, K, G = shape
    x0, goal, obst, noise = ec.scenes(N, no, K, G)
    margin, worst, winners = ec.SHAPE_MARGIN[shape], 0.0, []
    with make(mpc_gpu, N, no, G * K) as s:
        rig = Rig(mpc_gpu, torch, s, G, K, ec.OFFSETS[K], goal)
        rig.load(x0, obst)
        for k in range(ec.STEPS):
            rig.solve()
            pre = rig.snapshot()
            comp = rig.composed(pre, margin, noise[k])            # restarted from the fused path's read-back state, every step
            assert rig.tail(margin, noise[k]) == 0, rig.L.mpc_last_error()
            post = rig.snapshot()
            worst = max(worst, compare(rig, pre, post, comp, book_numpy(pre, comp, goal, G)))
            winners.append(post["winner"][:G].tolist())
            assert (post["steps"][:G] == k + 1).all() and (post["winner"][:G] >= 0).all()
    print(f"MULTISTART-EPISODES lockstep {shape}: winners per step {winners}; largest |fused - composed| over state, obstacles, seeded rows and margin {worst:.3e}")
    return worst


@pytest.mark.parametrize("shape", ec.SHAPES, ids=ec.SHAPE_IDS)
def test_the_tail_against_the_composition_in_lockstep(mg, shape):
    on_own_stream(lockstep, mg[0], shape)


# ---------------------------------------------------------------------------------------------------------------- 2. synthetic tables
def _synthetic(mg, K):
    import torch
    mpc_gpu, _ = mg
    N, no, G, margin = 20, 3, 6, 0.25
    rng = np.random.default_rng(31 + K)
    key = rng.uniform(20.0, 90.0, (G, K)); status = rng.choice(np.array([0, 0, 2, 4], np.int32), (G, K)).astype(np.int32)
    status[0] = 4                                                 # nobody eligible: u = 0, all K members seeded, lost counted, winner -1
    status[1] = 0; key[1, 0] = 10.0; key[1, 1:] = 9.0             # hysteresis keeps member 0 (9 is not below 0.75 x 10)
    status[2] = 0; key[2, 0] = 10.0; key[2, 1:] = 12.0; key[2, K - 1] = 7.0      # ... and here it is beaten, by the last member
    status[3] = 0; key[3] = 5.0; key[3, K // 2] = np.nan; key[3, 0] = 8.0        # a NaN key is not eligible; the rest tie below member 0, the tie goes to the lowest
    x0, goal, obst, noise = ec.scenes(N, no, K, G)
    with make(mpc_gpu, N, no, G * K) as s:
        rig = Rig(mpc_gpu, torch, s, G, K, np.linspace(-5.0, 5.0, K) if K > 5 else ec.OFFSETS[K], goal)
        rig.load(x0, obst, seed=False)
        B = G * K
        rig.X[:B] = rig.up(rng.uniform(-7, 7, (B, N + 1, 5))); rig.U[:B] = rig.up(rng.uniform(-3, 3, (B, N, 2))); rig.u0[:B] = rig.up(rng.uniform(-4, 4, (B, 2)))
        rig.key[:B] = rig.up(key.reshape(-1)); rig.status[:B] = rig.up(status.reshape(-1))
        pre = rig.snapshot()
        comp = rig.composed(pre, margin, noise[0])
        assert rig.tail(margin, noise[0]) == 0
        post = rig.snapshot()
        compare(rig, pre, post, comp, book_numpy(pre, comp, goal, G))
    w = post["winner"][:G]
    want = [mc.select(key[g], status[g], margin)[0] for g in range(G)]
    print(f"MULTISTART-EPISODES synthetic K={K}: winners {w.tolist()}")
    assert w.tolist() == want and w[0] == -1 and post["lost"][:G].tolist() == [int(v < 0) for v in want] and want[1:4] != [-1] * 3
    assert np.isinf(post["best_key"][0]) and not post["best_u0"][0].any()
    Xg, Ug = mc.guesses(post["x"][0], goal[0], rig.offsets, N)                                   # the lost group: every member seeded around the coasting state
    assert np.abs(post["X"][:K] - Xg).max() <= TOL and not post["U"][:K].any()
    if K > 1:
        assert w[1] == 0 and w[2] == K - 1 and w[3] == (1 if K // 2 != 1 else 2) and post["switched"][:4].tolist() == [0, 0, 1, 1]


@pytest.mark.parametrize("K", [1, 5, 64])
def test_synthetic_tables(mg, K):
    on_own_stream(_synthetic, mg, K)


# ---------------------------------------------------------------------------------------------------------------- 3. bookkeeping
def _bookkeeping(mg, feature):
    import torch
    mpc_gpu, _ = mg
    N, no, G, K = 5, 2, 5, 1
    goal = np.tile([5.0, 2.0], (G, 1))
    #        reaches the goal             leaves the arena             inside obstacle 0           clear                        clear, near obstacle 1
    x = np.array([[4.95, 1.9, 0.2, 0, 0], [7.95, 0.0, 0.0, 2.0, 0.0], [0.0, 0.4, 0.0, 0.0, 0.0], [-4.0, -4.0, 0.0, 0.5, 0.0], [2.0, -4.0, 0.0, 0.0, 0.0]])
    obst = np.tile(np.array([[0.5, 0.5, 0.0, 0.0], [4.0, -4.0, 0.0, 0.0]]), (G, 1, 1))
    r_hit = active = None
    margin_all = False
    with make(mpc_gpu, N, no, G * K) as s:
        if feature == "r_hit":                                    # group 2's obstacle 0 shrinks below the distance, group 4's obstacle 1 grows over it
            r_hit = np.full((G, no), ec.R_HIT); r_hit[2, 0] = 0.3; r_hit[4, 1] = 2.5
            s.set_instance_params(r_hit=r_hit)
        if feature in ("mask", "mask_all"):                       # group 2 does not see the obstacle it stands in
            active = np.ones((G, no), bool); active[2, 0] = False
            s.set_obstacle_mask(active)
            margin_all = feature == "mask_all"
        rig = Rig(mpc_gpu, torch, s, G, K, (0.0,), goal)
        rig.load(x, obst)
        rig.key[:G] = 1.0; rig.status[:G] = 0; rig.u0[:G] = 0.0
        pre = rig.snapshot()
        comp = rig.composed(pre, 0.0)
        assert rig.tail(0.0, flags=mpc_gpu._lib.GROUP_MARGIN_ALL if margin_all else 0) == 0, rig.L.mpc_last_error()
        post = rig.snapshot()
        book = book_numpy(pre, comp, goal, G, r_hit=r_hit, active=active, margin_all=margin_all)
        compare(rig, pre, post, comp, book)
    fl, st = post["flags"][:G].tolist(), post["steps"][:G].tolist()
    print(f"MULTISTART-EPISODES bookkeeping {feature}: flags {fl} steps {st} min_margin {post['min_margin'][:G].tolist()}")
    want = {"plain": [1, 2, 4, 0, 0], "r_hit": [1, 2, 0, 0, 4], "mask": [1, 2, 0, 0, 0], "mask_all": [1, 2, 4, 0, 0]}[feature]
    assert fl == want and st == [0, 1, 1, 1, 1]                   # the step that reaches the goal is not counted


@pytest.mark.parametrize("feature", ["plain", "r_hit", "mask", "mask_all"])
def test_bookkeeping_against_numpy(mg, feature):
    on_own_stream(_bookkeeping, mg, feature)


# ---------------------------------------------------------------------------------------------------------------- 4. idling
def _idling(mg, select_by):
    import torch
    mpc_gpu, _ = mg
    N, no, K = 20, 3, 3
    x0, goal, obst = (np.stack([a, a]) for a in mc.scene("C"))
    x0[0] = [3.95, 0.95, 0.1, 0.0, 0.0]                           # group 0 stands within the tolerance of its goal: the first step finishes it
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev(torch))
    c = lambda t: t.cpu().numpy().copy()
    with mpc_gpu.MultiStartMpc(N, no, 2.0, scenarios=2, offsets=ec.OFFSETS[K], select_by=select_by) as ms:
        x, ob, gl = up(x0), up(obst), up(goal)
        out = ms.step_fused(x, ob, gl)
        torch.cuda.synchronize()
        assert c(out["ep_flags"]).tolist() == [1, 0] and c(out["ep_steps"]).tolist() == [0, 1] and c(ms.member_flags).tolist() == [1] * K + [0] * K
        ms.cand_iters[:K] = -77                                   # the canary under the idle members' iteration words
        words = lambda: dict(x=c(x)[0], obst=c(ob)[0], X=c(ms.X)[:K], U=c(ms.U)[:K], mm=c(ms.min_margin)[0], fl=c(ms.ep_flags)[0], st=c(ms.ep_steps)[0],
                             lost=c(ms.lost_steps)[0], sw=c(ms.switched_steps)[0], it=c(ms.cand_iters)[:K], mx=c(ms._x0)[0], mo=c(ms._obst)[0], mf=c(ms.member_flags)[:K],
                             cost=c(ms.cand_cost)[:K], status=c(ms.cand_status)[:K], u0=c(ms.cand_u0)[:K], w=c(ms.winner)[0], bu=c(ms.u0)[0],
                             sm=c(ms._scratch_margin)[:K], ss=c(ms._scratch_steps)[:K])
        before, live = words(), (c(x)[1], c(ob)[1], c(ms.X)[K:])
        for _ in range(2):
            out = ms.step_fused(x, ob, gl)
        torch.cuda.synchronize()
        after = words()
        for n in before:
            assert np.array_equal(before[n], after[n], equal_nan=True), n
        assert after["it"].tolist() == [-77] * K
        assert c(out["ep_steps"]).tolist() == [0, 3] and c(out["ep_flags"])[1] & 1 == 0                      # the neighbour in the same workgroup steps on
        assert np.abs(c(x)[1] - live[0]).max() > 1e-3 and np.abs(c(ob)[1] - live[1]).max() > 1e-3 and np.abs(c(ms.X)[K:] - live[2]).max() > 1e-3
        assert (c(ms.cand_iters)[K:] > 0).all() and (c(ms._x0)[1] == c(x)[1]).all()


@pytest.mark.parametrize("select_by", ["cost", "rollout"])
def test_a_finished_group_idles_and_its_neighbour_steps_on(mg, select_by):
    on_own_stream(_idling, mg, select_by)


# ---------------------------------------------------------------------------------------------------------------- 5. the driver
def _python_loop(mpc_gpu, torch, x0, goal, obst, noise, offsets, margin, N, Tf, max_iter):
    """scripts/multistart_rate.py's closed_loop over MultiStartMpc.step: the bookkeeping by hand, in torch"""
    G, no = obst.shape[0], obst.shape[1]
    dev = _dev(torch)
    with mpc_gpu.MultiStartMpc(N, no, Tf, scenarios=G, offsets=offsets, incumbent_margin=margin) as ms:
        with torch.cuda.stream(ms.stream):
            x, gl, ob, nz = (torch.from_numpy(a.copy()).to(dev) for a in (x0, goal, obst, noise))
            reached = torch.zeros(G, dtype=torch.bool, device=dev); steps = torch.zeros(G, dtype=torch.int32, device=dev)
            mm = torch.full((G,), float("inf"), dtype=torch.float64, device=dev)
            lost, sw, oob = (torch.zeros(G, dtype=torch.int32, device=dev) for _ in range(3))
            x_last = x.clone()
            for k in range(max_iter):
                res = ms.step(x, ob, gl, noise=nz[k])
                live = ~reached
                d = torch.linalg.norm(x[:, None, :2] - ob[:, :, :2], dim=2).min(dim=1).values - ec.R_HIT
                mm = torch.where(live, torch.minimum(mm, d), mm)
                lost += (live & (res["winner"] < 0)).int(); sw += (live & (res["winner"] > 0)).int()
                oob |= (live & ((x[:, 0].abs() > 8.0) | (x[:, 1].abs() > 8.0))).int()
                now = torch.linalg.norm(x[:, :2] - gl, dim=1) <= ec.TOL_GOAL
                steps += (live & ~now).int()
                x_last = torch.where(live[:, None], x, x_last)
                reached |= now
            torch.cuda.synchronize()
            c = lambda t: t.cpu().numpy()
            fl = c(reached).astype(np.int32) | (c(oob) << 1) | ((c(mm) <= 0).astype(np.int32) << 2)
            return dict(flags=fl, steps=c(steps), min_margin=c(mm), lost=c(lost), switched=c(sw), x_last=c(x_last))


def _driver(mg):
    import torch
    mpc_gpu, _ = mg
    from mpc_gpu import world
    d = ec.DRIVER
    x0, goal, obst, noise = ec.driver_inputs(world)
    run = lambda: mpc_gpu.run_multistart_episodes(x0, goal, obst, offsets=ec.OFFSETS[d["K"]], incumbent_margin=d["margin"], N=d["N"], Tf=d["Tf"],
                                                  max_iter=d["max_iter"], noise=noise)
    r1, r2 = run(), run()
    for k in r1:
        assert np.array_equal(r1[k], r2[k], equal_nan=True), k                                   # a second run gives the same bits
    py = _python_loop(mpc_gpu, torch, x0, goal, obst, noise, ec.OFFSETS[d["K"]], d["margin"], d["N"], d["Tf"], d["max_iter"])
    from mpc_gpu.episodes import result_table
    want = result_table(py["flags"], py["min_margin"], py["x_last"], goal, py["steps"])
    print(f"MULTISTART-EPISODES driver: table\n{r1['table']}\nlargest |driver - python loop| {np.abs(r1['table'] - want).max():.3e}; lost {r1['lost_steps']} switched {r1['switched_steps']}")
    assert np.array_equal(r1["table"][:, [0, 1, 4, 5]], want[:, [0, 1, 4, 5]])                   # flags and steps equal
    assert np.array_equal(r1["lost_steps"], py["lost"]) and np.array_equal(r1["switched_steps"], py["switched"])
    assert np.abs(r1["table"] - want).max() <= 1e-9 and np.abs(r1["x_last"] - py["x_last"]).max() <= 1e-9
    assert r1["steps_run"] == d["max_iter"] and r1["solves"] == d["K"] * int(r1["table"][:, 4].sum() + r1["table"][:, 1].sum()) == d["K"] * d["G"] * d["max_iter"]
    assert r1["switched_steps"].sum() > 0


def test_the_driver_against_the_python_loop(mg):
    on_own_stream(_driver, mg)


def _driver_ends_early(mg):
    mpc_gpu, _ = mg
    G, K = 5, 3
    goal = np.array([2.0, 1.0])
    x0 = np.array([[2.0 - 0.3 - 0.1 * g, 1.0 - 0.2, 0.4, 0.0, 0.0] for g in range(G)])
    obst = np.tile(np.array([[-6.5, 6.5, 0.0, 0.0]]), (G, 1, 1))                                  # nothing in the way
    r = mpc_gpu.run_multistart_episodes(x0, goal, obst, offsets=ec.OFFSETS[K], max_iter=2000, random_move=False)
    print(f"MULTISTART-EPISODES early end: steps_run {r['steps_run']} episode steps {r['table'][:, 4].tolist()} solves {r['solves']}")
    assert (r["table"][:, 1] == 1).all() and (r["table"][:, 0] == 0).all() and (r["table"][:, 5] == 0).all()
    assert (r["table"][:, 3] <= ec.TOL_GOAL).all()
    assert r["table"][:, 4].max() < r["steps_run"] < 2000         # the loop saw the done flag (the host queues ahead of the device: how far is not asserted)
    assert r["solves"] == int(sum(K * (st + re) for st, re in zip(r["table"][:, 4], r["table"][:, 1])))


def test_the_driver_ends_early_when_every_group_has_reached_its_goal(mg):
    on_own_stream(_driver_ends_early, mg)


# ---------------------------------------------------------------------------------------------------------------- 6. argument errors
def _refusals(mg):
    import torch
    mpc_gpu, _ = mg
    ERR = mpc_gpu._lib.MPC_ERR_ARG
    N, no, G, K = 5, 2, 2, 3
    x0, goal, obst, _ = ec.scenes(N, no, K, G)
    with make(mpc_gpu, N, no, G * K) as s:
        rig = Rig(mpc_gpu, torch, s, G, K, ec.OFFSETS[K], goal)
        rig.load(x0, obst)
        rig.key[:G * K] = 1.0; rig.status[:G * K] = 0; rig.u0[:G * K] = 0.0
        pre = rig.snapshot()
        O = mpc_gpu._lib.GroupStepOut
        fields = {n: getattr(rig.out, n) for n, _ in O._fields_}
        without = lambda n: O(**{k: v for k, v in fields.items() if k != n})
        cases = [(dict(K=0), b"K must be"), (dict(K=65), b"K must be"), (dict(G=3), b"max_batch"), (dict(G=-1), b"max_batch"), (dict(h=None), b"null handle"),
                 (dict(out=None), b"null")] + [({n: None}, b"null") for n in ("key", "status", "u0", "x", "obst", "goal", "off", "X", "U")] \
            + [(dict(out=without(n)), b"in out") for n in ("winner", "min_margin", "ep_flags", "ep_steps")]
        for kw, word in cases:
            assert rig.tail(0.0, **kw) == ERR and word in rig.L.mpc_last_error(), (kw, rig.L.mpc_last_error())
        for m in (-0.01, 1.0, float("nan")):
            assert rig.tail(m) == ERR and b"incumbent_margin" in rig.L.mpc_last_error()
        assert rig.tail(0.0, flags=2) == ERR and b"flags" in rig.L.mpc_last_error()
        post = rig.snapshot()
        for n in pre:
            assert np.array_equal(pre[n], post[n], equal_nan=True), n                             # nothing was launched
        assert rig.bd.intact()
        # what is allowed: no groups; every optional output absent
        assert rig.tail(0.0, G=0) == 0
        assert rig.tail(0.0, out=O(**{k: v for k, v in fields.items() if k in ("winner", "min_margin", "ep_flags", "ep_steps")})) == 0
        last = rig.snapshot()
        assert last["steps"][:G].tolist() == [1, 1] and np.array_equal(last["mx"], pre["mx"]) and np.array_equal(last["best_key"], pre["best_key"])


def test_refusals_and_optional_outputs(mg):
    on_own_stream(_refusals, mg)
