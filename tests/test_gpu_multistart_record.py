"""The per-group closed-loop record of multi-start episodes on the GPU (mpc_group_record_set_dev / mpc_group_record_dev, MultiStartMpc.group_record_set_dev,
run_multistart_episodes(record=)).  The yardsticks are the numpy restatement of the two phases (multistart_record_cases.solved / stepped) and, for the driver,
the path that exists without the feature: multistart_record_cases.clone_loop, the test's own loop over the entry points that were there before it with clones
behind each launch; never the new kernel itself.

  1. the C ABI on hand-made inputs under guard bands, at (N, n_obst, K, G) = (2, 1, 1, 3), (20, 5, 3, 5), (62, 10, 2, 3), (31, 12, 3, 2), (2, 1, 64, 2): random X,
     keys and status words, groups that run, idle, reach their goal in this step, solve their last step and are not recorded, permuted rows and a row nobody
     owns, the record prefilled with sentinels: both phases bit for bit against the restatement (so every word a phase does not write still holds its sentinel),
     every input unchanged; again with cand_X NULL;
  2. every refusal with all arrays unchanged, mpc_group_refill_dev's with a record attached, and the refill accepted again once it is detached;
  3. the sweep scene of test_multistart_sweep_host.py (N 20, 5 obstacles, K 3, seeds 40 .. 48, max_iter 25; its oracle-alone conditions are asserted there):
     run_multistart_episodes(record=True) against the clone loop, every recorded array bit for bit; table, x_last, lost and switched steps those of the run
     without a record bit for bit; the recorded winner the selection rule's on the recorded keys; a subset, no plans, the rollout merit, the guess geometry, a
     caller's handle that leaves detached, and a failing attach or step."""
import ctypes as C

import numpy as np
import pytest

import multistart_cases as mc
import multistart_episode_cases as ec
import multistart_record_cases as rc
import multistart_sweep_cases as sc
from feature_loop import Banded, make, mg, on_own_stream      # noqa: F401 (mg is a fixture)

pytestmark = pytest.mark.gpu
T_ABI = 4


def _dev(torch):
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Rig:
    """the inputs of mpc_group_record_dev and the record arrays for one set of made-up group words, each between guard bands"""

    def __init__(self, mpc_gpu, torch, s, inp, group_row, rec, K, T):
        self.mpc_gpu, self.torch, self.s, self.K, self.T, self.G = mpc_gpu, torch, s, K, T, len(group_row)
        self.bd = Banded(torch, _dev(torch))
        alloc = lambda a: (self.bd.f64 if a.dtype == np.float64 else self.bd.i32)(*a.shape)
        self.inp = {n: alloc(a) for n, a in inp.items()}
        self.rec = {n: alloc(a) for n, a in rec.items()}
        self.group_row = alloc(group_row)
        self.put(self.inp, inp); self.put(self.rec, rec); self.put(dict(r=self.group_row), dict(r=group_row))
        self.out = mpc_gpu._lib.GroupStepOut(winner=self.inp["winner"].data_ptr(), best_key=self.inp["best_key"].data_ptr(), best_u0=self.inp["best_u0"].data_ptr(),
                                             ep_flags=self.inp["ep_flags"].data_ptr(), ep_steps=self.inp["ep_steps"].data_ptr())
        self.L = mpc_gpu._lib.lib()
        self.q = torch.cuda.current_stream().cuda_stream

    def sync(self):
        self.torch.cuda.current_stream().synchronize()

    def put(self, dst, src):
        for n, a in src.items():
            dst[n].copy_(self.torch.from_numpy(np.ascontiguousarray(a)))
        self.sync()

    def host(self, d):
        self.sync()
        return {n: t.cpu().numpy().copy() for n, t in d.items()}

    def attach(self, plans=True, **kw):
        f = dict(group_row=self.group_row, **{n: t for n, t in self.rec.items() if plans or n != "cand_X"})
        f.update(kw)
        rows, max_steps, K = f.pop("rows", self.rec["len"].shape[0]), f.pop("max_steps", self.T), f.pop("K", self.K)
        h = f.pop("h", self.s._h)
        r = self.mpc_gpu._lib.GroupRecord(**{n: (None if t is None else t.data_ptr()) for n, t in f.items()})
        return self.L.mpc_group_record_set_dev(h, rows, max_steps, K, C.byref(r))

    def call(self, phase, **kw):
        a = dict(h=self.s._h, G=self.G, K=self.K, phase=phase, out=C.byref(self.out), **{n: _p(self.inp[n]) for n in ("x", "obst", "X", "key", "status", "iters", "u0")})
        a.update(kw)
        rc_ = self.L.mpc_group_record_dev(a["h"], a["G"], a["K"], a["phase"], a["x"], a["obst"], a["X"], a["key"], a["status"], a["iters"], a["u0"], a["out"], self.q)
        self.sync()
        return rc_


def _same(a, b):
    return all(np.array_equal(a[n], b[n]) for n in a) and sorted(a) == sorted(b)


# ---------------------------------------------------------------------------------------------------------------- 1. the C ABI against the restatement
SHAPES = [(2, 1, 1, 3), (20, 5, 3, 5), (62, 10, 2, 3), (31, 12, 3, 2), (2, 1, 64, 2)]
SHAPE_IDS = ["N%d-no%d-K%d-G%d" % s for s in SHAPES]


def _abi(mg, shape, plans):
    import torch
    mpc_gpu, _ = mg
    N, no, K, G = shape
    seen = set()
    with make(mpc_gpu, N, no, G * K) as s:
        for shift in range(0, len(rc.ROLES), G):                  # every role a group can be in, G at a time
            roles = [rc.ROLES[(shift + g) % len(rc.ROLES)] for g in range(G)]
            seen.update(roles)
            rng = np.random.default_rng(1000 * N + 10 * K + shift)
            inp, group_row, rec0 = rc.made_up(roles, T_ABI, K, N, no, rng)
            if not plans:
                del rec0["cand_X"]
            rig = Rig(mpc_gpu, torch, s, inp, group_row, rec0, K, T_ABI)
            assert rig.attach(plans=plans) == 0, rig.L.mpc_last_error()
            # SOLVED, on what the member solve left
            want = rc.solved(rec0, group_row, T_ABI, inp, K)
            assert rig.call(rc.SOLVED) == 0, rig.L.mpc_last_error()
            got = rig.host(rig.rec)
            assert _same(got, want), [n for n in want if not np.array_equal(got[n], want[n])]
            assert _same(rig.host(rig.inp), inp) and np.array_equal(rig.group_row.cpu().numpy(), group_row) and rig.bd.intact()
            # the group tail (made up on the host: it overwrites the members' iterates), then STEPPED
            after = rc.fake_tail(inp, roles, K, rng)
            rig.put(rig.inp, after)
            want2 = rc.stepped(want, group_row, T_ABI, after, K)
            assert rig.call(rc.STEPPED) == 0, rig.L.mpc_last_error()
            got = rig.host(rig.rec)
            assert _same(got, want2), [n for n in want2 if not np.array_equal(got[n], want2[n])]
            assert _same(rig.host(rig.inp), after) and np.array_equal(rig.group_row.cpu().numpy(), group_row) and rig.bd.intact()
            # the restatement itself wrote what the case is about, and the rows of idle and unrecorded groups and the row nobody owns hold their sentinels
            owned = set()
            for g, role in enumerate(roles):
                r = group_row[g]
                if role == "unrec":
                    assert r == -1
                    continue
                owned.add(int(r))
                if role == "idle":
                    assert all(np.array_equal(got[n][r], rec0[n][r]) for n in got), role
                    assert all((got[n][r] == (rc.F_SENT if got[n].dtype == np.float64 else rc.I_SENT)).all() for n in got if n != "len")
                else:
                    t = int(inp["ep_steps"][g])
                    assert got["len"][r] == t + 1 and np.array_equal(got["x"][r, t], inp["x"][g]) and np.array_equal(got["x"][r, t + 1], after["x"][g])
                    assert got["winner"][r, t] == after["winner"][g] and np.array_equal(got["cand_key"][r, t], inp["key"][g * K:(g + 1) * K])
                    if plans:
                        assert np.array_equal(got["cand_X"][r, t], inp["X"][g * K:(g + 1) * K]) and not np.array_equal(inp["X"], after["X"])
            for r in set(range(rec0["len"].shape[0])) - owned:
                assert all((got[n][r] == (rc.F_SENT if got[n].dtype == np.float64 else rc.I_SENT)).all() for n in got)
            # a second STEPPED launch writes nothing
            assert rig.call(rc.STEPPED) == 0 and _same(rig.host(rig.rec), want2)
            assert s.group_record_set_dev(0) is None
    assert seen == set(rc.ROLES)


@pytest.mark.parametrize("plans", [True, False], ids=["plans", "no-plans"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_both_phases_against_the_restatement(mg, shape, plans):
    on_own_stream(_abi, mg, shape, plans)


# ---------------------------------------------------------------------------------------------------------------- 2. the refusals
def _refusals(mg):
    import torch
    mpc_gpu, _ = mg
    from test_gpu_multistart_sweep import Rig as RefillRig, sc_rows
    ERR = mpc_gpu._lib.MPC_ERR_ARG
    N, no, K, G, T = 5, 2, 3, 2, T_ABI
    rng = np.random.default_rng(4)
    roles = ["run", "reach"]
    inp, group_row, rec0 = rc.made_up(roles, T, K, N, no, rng)
    with make(mpc_gpu, N, no, 3 * K) as s:
        rig = Rig(mpc_gpu, torch, s, inp, group_row, rec0, K, T)
        L = rig.L
        unchanged = lambda: _same(rig.host(rig.rec), rec0) and _same(rig.host(rig.inp), inp) and rig.bd.intact()
        assert rig.call(rc.SOLVED) == ERR and b"no record attached" in L.mpc_last_error()
        for kw, word in [(dict(h=None), b"null handle"), (dict(rows=-1), b"rows"), (dict(max_steps=0), b"max_steps"), (dict(K=0), b"K must be"), (dict(K=65), b"K must be")] \
                + [({n: None}, n.encode() + b" is null") for n in rc.FIELDS if n != "cand_X"]:
            assert rig.attach(**kw) == ERR and word in L.mpc_last_error(), (kw, L.mpc_last_error())
        assert rig.call(rc.SOLVED) == ERR and b"no record attached" in L.mpc_last_error()          # a refused attach attaches nothing
        assert rig.attach() == 0
        O = mpc_gpu._lib.GroupStepOut
        fields = {n: getattr(rig.out, n) for n, _ in O._fields_}
        without = lambda n: C.byref(O(**{k: v for k, v in fields.items() if k != n}))
        cases = [(dict(h=None), b"null handle"), (dict(phase=2), b"phase"), (dict(phase=-1), b"phase"), (dict(G=0), b"groups"), (dict(G=-1), b"groups"),
                 (dict(G=4), b"max_batch"), (dict(K=2), b"K differs"), (dict(K=0), b"K must be"), (dict(K=65), b"K must be"), (dict(out=None), b"out is null")] \
            + [({n: None}, b"d_" + n.encode() + b" is null") for n in ("x", "obst", "X", "key", "status", "iters", "u0")] \
            + [(dict(out=without(n)), n.encode()) for n in ("winner", "ep_flags", "ep_steps")]
        for phase in (rc.SOLVED, rc.STEPPED):
            for kw, word in cases:
                assert rig.call(**dict(dict(phase=phase), **kw)) == ERR and word in L.mpc_last_error(), (kw, L.mpc_last_error())
        for n in ("best_key", "best_u0"):
            assert rig.call(rc.STEPPED, out=without(n)) == ERR and b"STEPPED" in L.mpc_last_error()
        assert unchanged()
        # SOLVED reads neither best_key nor best_u0: it is taken without them
        assert rig.call(rc.SOLVED, out=without("best_key")) == 0 and _same(rig.host(rig.rec), rc.solved(rec0, group_row, T, inp, K))
        rig.put(rig.rec, rec0)
        # the refill for groups refuses a handle that holds a record, and writes nothing; detached, it is taken again
        count = 3
        start, goal_rows = sc_rows(count, rng)
        refill = RefillRig(mpc_gpu, torch, s, G, K, count, ec.OFFSETS[K], start, goal_rows)
        pre = refill.snapshot()
        assert refill.call() == ERR and b"not offered for groups" in L.mpc_last_error() and b"mpc_group_record_set_dev" in L.mpc_last_error()
        post = refill.snapshot()
        assert all(np.array_equal(pre[n], post[n], equal_nan=True) for n in pre) and refill.bd.intact() and unchanged()
        assert s.group_record_set_dev(0) is None
        assert rig.call(rc.STEPPED) == ERR and b"no record attached" in L.mpc_last_error()
        assert refill.call() == 0, L.mpc_last_error()
        assert refill.snapshot()["slot_seed"].tolist() == [0, 1] and unchanged()


def test_refusals_leave_every_array_unchanged(mg):
    on_own_stream(_refusals, mg)


# ---------------------------------------------------------------------------------------------------------------- 3. the scene against the clone loop
def _problem():
    d = sc.SWEEP
    return dict(offsets=ec.OFFSETS[d["K"]], incumbent_margin=d["margin"], N=d["N"], Tf=d["Tf"], n_obst=d["no"], max_iter=d["max_iter"])


def _run(mpc_gpu, **kw):
    d = sc.SWEEP
    return mpc_gpu.run_multistart_episodes(sc.START, sc.GOAL, d["scenario"], first_seed=d["first_seed"], **_problem(), **kw)


def _yardstick(mpc_gpu, select_by="cost", guess_geometry=None):
    d = sc.SWEEP
    return rc.clone_loop(mpc_gpu, sc.START, sc.GOAL, d["scenario"], d["first_seed"], _problem(), select_by=select_by, guess_geometry=guess_geometry)


NAMES = ("simX", "obst_traj", "u", "winner", "key", "cand_key", "cand_status", "cand_iters", "cand_u0", "cand_X")


def assert_record_is(r, ref, groups, plans=True, margin=0.0):
    d = sc.SWEEP
    assert sorted(r["record"]) == sorted(groups)
    lengths = (r["table"][:, 4] + r["table"][:, 1]).astype(np.int64)
    for g in groups:
        t, want, L = r["record"][g], ref["record"][g], int(lengths[g])
        assert sorted(t) == sorted(n for n in NAMES if plans or n != "cand_X"), g
        assert t["u"].shape == (L, 2) and t["simX"].shape == (L + 1, 5) and t["obst_traj"].shape == (L + 1, d["no"], 4) and t["winner"].shape == (L,)
        assert t["cand_key"].shape == (L, d["K"]) and t["cand_u0"].shape == (L, d["K"], 2) and (not plans or t["cand_X"].shape == (L, d["K"], d["N"] + 1, 5))
        for n in t:
            assert t[n].dtype == want[n].dtype and np.array_equal(t[n], want[n]), (g, n)            # bit for bit
        # the recorded choice is the selection rule's on the recorded candidates, and the input applied is the winner's
        w, key, u = mc.select_groups(t["cand_key"], t["cand_status"], margin, u0=t["cand_u0"])
        assert np.array_equal(t["winner"], w) and np.array_equal(t["key"], key) and np.array_equal(t["u"], u), g
        assert np.array_equal(t["simX"][-1], r["x_last"][g])


def _scene(mg, select_by, geometry):
    mpc_gpu, _ = mg
    d = sc.SWEEP
    kw = dict(select_by=select_by, guess_geometry=geometry)
    ref = _yardstick(mpc_gpu, select_by, geometry)
    plain = _run(mpc_gpu, **kw)
    r = _run(mpc_gpu, record=True, **kw)
    lengths = (plain["table"][:, 4] + plain["table"][:, 1]).astype(np.int64)
    print(f"MULTISTART-RECORD by {select_by}, geometry {geometry}: lengths {lengths.tolist()}, lost {plain['lost_steps'].tolist()}, switched {plain['switched_steps'].tolist()}")
    assert "record" not in plain
    for other in (plain, ref):
        for n in ("table", "x_last", "lost_steps", "switched_steps"):
            assert np.array_equal(r[n], other[n]), n
    assert r["solves"] == plain["solves"] and len(set(lengths.tolist())) >= 3 and (plain["table"][:, 1] == 1).any() and (plain["table"][:, 1] == 0).any()
    assert_record_is(r, ref, range(d["count"]))
    sw = sum(int((r["record"][g]["winner"] > 0).sum()) for g in range(d["count"]))
    assert sw == int(plain["switched_steps"].sum()) and all(int((r["record"][g]["winner"] < 0).sum()) == plain["lost_steps"][g] for g in range(d["count"]))
    if geometry is None and select_by == "cost":
        # a subset in the order given, and without plans
        sub = _run(mpc_gpu, record=[7, 0, 3], **kw)
        assert_record_is(sub, ref, [0, 3, 7])
        assert np.array_equal(sub["table"], plain["table"]) and np.array_equal(sub["x_last"], plain["x_last"])
        nop = _run(mpc_gpu, record=True, record_plans=False, **kw)
        assert_record_is(nop, ref, range(d["count"]), plans=False)
        with pytest.raises(ValueError, match="record_plans=False"):
            mpc_gpu.multistart_record(nop, 4)
        v = mpc_gpu.visualisation_inputs(mpc_gpu.multistart_record(r, 4), 0)
        L = int(lengths[4])
        assert v["trajectory"].shape == (2, L + 1) and v["pred"].shape == (L + 1, d["N"] + 1, 2) and len(v["obstacles"]) == d["no"]
        t = r["record"][4]
        # (stage 0 of the re-assembled horizon is the plant state the solve started from; stages 1 .. N are the winner's solved plan)
        assert all(np.array_equal(v["pred"][j + 1, 1:], t["cand_X"][j, max(int(t["winner"][j]), 0)][1:, :2]) for j in range(L))
        assert all(np.array_equal(v["pred"][j + 1, 0], t["simX"][j, :2]) for j in range(L))


@pytest.mark.parametrize("select_by, geometry", [("cost", None), ("rollout", None), ("cost", True)], ids=["cost", "rollout", "geometry"])
def test_the_record_against_the_clone_loop(mg, select_by, geometry):
    on_own_stream(_scene, mg, select_by, geometry)


def _assert_detached(mpc_gpu, ms):
    import torch
    assert not ms._recording
    z = torch.zeros(ms.B * (ms.N + 1) * 5, dtype=torch.float64, device=ms.dev); w = torch.zeros(ms.B, dtype=torch.int32, device=ms.dev)
    ms._group_arrays()
    with pytest.raises(mpc_gpu._lib.MpcError, match="no record attached"):
        ms.inner.group_record_dev(ms.G, ms.K, rc.SOLVED, z, z, z, z, w, w, z, ms._out)
    torch.cuda.synchronize()


def _callers_solver(mg):
    mpc_gpu, _ = mg
    d = sc.SWEEP
    ref = _yardstick(mpc_gpu)
    p = _problem()
    with mpc_gpu.MultiStartMpc(d["N"], d["no"], d["Tf"], scenarios=d["count"], offsets=p["offsets"], incumbent_margin=d["margin"]) as ms:
        r = _run(mpc_gpu, solver=ms, record=[2, 8])
        shapes = dict(ms.inner.group_record_shapes)
        _assert_detached(mpc_gpu, ms)
        again = _run(mpc_gpu, solver=ms)
        assert "record" not in again and np.array_equal(again["table"], ref["table"]) and np.array_equal(again["x_last"], ref["x_last"])
        assert_record_is(r, ref, [2, 8])
        T, K, N, no = d["max_iter"], d["K"], d["N"], d["no"]
        assert shapes == dict(group_row=(9,), len=(2,), x=(2, T + 1, 5), obst=(2, T + 1, no, 4), u=(2, T, 2), winner=(2, T), best_key=(2, T), cand_key=(2, T, K),
                              cand_status=(2, T, K), cand_iters=(2, T, K), cand_u0=(2, T, K, 2), cand_X=(2, T, K, N + 1, 5))
        # a failing attach, then a failing step (the second STEPPED launch), injected in Python: the handle leaves detached, and runs on
        def refuse(*a, **kw):
            raise mpc_gpu._lib.MpcError("injected refusal")
        ms.inner.group_record_set_dev = lambda *a, **kw: refuse() if a and a[0] else type(ms.inner).group_record_set_dev(ms.inner, *a, **kw)
        with pytest.raises(mpc_gpu._lib.MpcError, match="injected refusal"):
            _run(mpc_gpu, solver=ms, record=True)
        del ms.inner.group_record_set_dev
        _assert_detached(mpc_gpu, ms)
        calls = []
        launch = ms.inner.group_record_dev
        ms.inner.group_record_dev = lambda *a, **kw: refuse() if len(calls) == 3 else (calls.append(1), launch(*a, **kw))[1]
        with pytest.raises(mpc_gpu._lib.MpcError, match="injected refusal"):
            _run(mpc_gpu, solver=ms, record=True)
        del ms.inner.group_record_dev
        assert len(calls) == 3, "the case itself: the record was attached and launching when the step failed"
        _assert_detached(mpc_gpu, ms)
        again = _run(mpc_gpu, solver=ms, record=[5])
        assert_record_is(again, ref, [5])
        assert np.array_equal(again["table"], ref["table"]) and np.array_equal(again["x_last"], ref["x_last"])


def test_a_callers_solver_leaves_detached_on_return_and_on_failure(mg):
    on_own_stream(_callers_solver, mg)
