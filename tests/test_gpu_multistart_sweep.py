"""The refill for multi-start groups and its sweep driver on the GPU (mpc_group_refill_dev, MultiStartMpc.members_loaded, run_multistart_sweep).  The
yardsticks are the numpy restatement of the rule (multistart_sweep_cases), the entry points that existed before it -- mpc_generate_scenarios_dev,
mpc_noise_init_dev, mpc_seed_guesses_dev -- and, for the driver, run_multistart_episodes on ONE batch holding every seed; never the new kernel itself.

  1. the C ABI on preset arrays under guard bands, at (N, n_obst, K, G) = (2, 1, 1, 3), (20, 5, 3, 5), (62, 10, 2, 3), (31, 12, 3, 2) and K = 64 with one group:
     the first call from the preset state fills every group; a call with nothing finished writes nothing; a call that mixes kept groups, groups finished by
     their flag and groups finished by their budget, of which the last is drained where two or more have finished; a last call in which every running group
     ends on its budget and is drained.  Kept groups and every input bit for bit; parked rows, bookkeeping, slot_seed, cursor, member_flags exact; a started
     group's obstacle states and generator state those of the existing entry points bit for bit; its X within 1e-12 of mpc_seed_guesses_dev (the project's
     tolerance for guesses: two kernels that inline seed_stage may differ by an ulp), X[0] and U exact; the member inputs the group's rows exactly;
  2. more group slots than seeds; the refusals, with every array unchanged;
  3. the sweep scene of test_multistart_sweep_host.py (which holds it to the conditions that make the comparison fair) through 4 group slots, and through 2
     with select_by="rollout", against the batch of its 9 groups: flags, step counts, lost and switched steps equal, table and x_last within 1e-9 (the bound
     test_gpu_multistart_episodes.py holds the batch driver to: three member solves share a wavefront, and an episode's rounding depends on its neighbours),
     solves, the schedule, a second run with the same bits, fewer control steps than seed after seed, and a caller's handle that leaves as it came."""
import ctypes as C

import numpy as np
import pytest

import multistart_episode_cases as ec
import multistart_sweep_cases as sc
from feature_loop import Banded, make, mg, on_own_stream      # noqa: F401 (mg is a fixture)

pytestmark = pytest.mark.gpu
TOL = 1e-12          # the project's tolerance for guesses (test_gpu_multistart.py)
MAX_STEPS = 7
FIRST = 37
SCEN_ID = {"RANDOM": 0, "CENTER": 1, "EDGE": 2}


def _dev(torch):
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Rig:
    """every array of mpc_group_refill_dev for G groups of K members and `count` seeds on a BatchedMpc `s`, each between guard bands, preset as the first
    call of a sweep wants them; host copies in the restatement's layout"""

    def __init__(self, mpc_gpu, torch, s, G, K, count, offsets, start, goal_rows, scenario="RANDOM"):
        self.mpc_gpu, self.torch, self.s, self.G, self.K, self.count, self.scenario = mpc_gpu, torch, s, G, K, count, scenario
        self.N, self.no = s.N, s.n_obst
        self.bd = Banded(torch, _dev(torch))
        for n, (_, _, dt) in sc.ARRAYS.items():
            setattr(self, n, (self.bd.f64 if dt == "f8" else self.bd.i32)(*sc.shape_of(n, G, K, count, self.N, self.no)))
        self.offsets = tuple(offsets)
        self.start_h, self.goal_h = np.atleast_2d(np.asarray(start, dtype=np.float64)), np.atleast_2d(np.asarray(goal_rows, dtype=np.float64))
        self.per_seed = self.start_h.shape[0] > 1
        self.inputs = {}
        for n, a in (("start", self.start_h), ("goal_rows", self.goal_h), ("off", np.asarray(offsets, dtype=np.float64))):
            self.inputs[n] = self.bd.f64(*a.shape); self.inputs[n].copy_(torch.from_numpy(np.ascontiguousarray(a)))
        self.box = mpc_gpu.BatchedMpc._scenario_box()
        self.arr = mpc_gpu._lib.GroupRefillArrays(**{n: getattr(self, n).data_ptr() for n in sc.ARRAYS})
        self.q = torch.cuda.current_stream().cuda_stream
        self.L = mpc_gpu._lib.lib()
        self.put(sc.first_call(G, K, count, self.N, self.no))

    def sync(self):
        self.torch.cuda.current_stream().synchronize()

    def put(self, a):
        for n in sc.ARRAYS:
            h = np.ascontiguousarray(a[n])
            getattr(self, n).copy_(self.torch.from_numpy(h.view(np.int32) if h.dtype == np.uint32 else h))
        self.sync()

    def snapshot(self):
        self.sync()
        out = {n: getattr(self, n).cpu().numpy().copy() for n in sc.ARRAYS}
        out["state"] = out["state"].view(np.uint32)
        return out

    def inputs_host(self):
        self.sync()
        return {n: t.cpu().numpy().copy() for n, t in self.inputs.items()}

    def call(self, **kw):
        a = dict(h=self.s._h, G=self.G, K=self.K, scenario=SCEN_ID[self.scenario], first=FIRST, count=self.count, max_steps=MAX_STEPS, box=self.box.ctypes.data,
                 start=_p(self.inputs["start"]), goal_rows=_p(self.inputs["goal_rows"]), per_seed=1 if self.per_seed else 0, off=_p(self.inputs["off"]), arr=self.arr)
        a.update(kw)
        rc = self.L.mpc_group_refill_dev(a["h"], a["G"], a["K"], a["scenario"], a["first"], a["count"], a["max_steps"], a["box"], a["start"], a["goal_rows"],
                                         a["per_seed"], a["off"], a["arr"], self.q)
        self.sync()
        return rc

    def model(self, world, pre):
        return sc.refill(world, pre, self.K, self.N, self.offsets, self.scenario, FIRST, self.count, MAX_STEPS, self.start_h, self.goal_h, self.per_seed)

    def references(self):
        """what the entry points that existed before the refill give for every seed index: obstacle states (count, no, 4), generator states (count, words)
        and the guess family (count, K, N + 1, 5), (count, K, N, 2) around each seed's start and goal row"""
        torch, s, c, K = self.torch, self.s, self.count, self.K
        f64 = lambda *sh: torch.zeros(*sh, dtype=torch.float64, device=_dev(torch))
        obst, X, U = f64(c, self.no, 4), f64(c * K, self.N + 1, 5), f64(c * K, self.N, 2)
        s.generate_scenarios_dev(self.scenario, c, obst, seed0=FIRST, stream=self.q)
        state = s.noise_state(c, self.scenario, seed0=FIRST, stream=self.q)
        rows = lambda a: torch.from_numpy(np.array(np.broadcast_to(a, (c, a.shape[1])), order="C")).to(_dev(torch))
        x0, gl = rows(self.start_h), rows(self.goal_h)
        assert self.L.mpc_seed_guesses_dev(s._h, c, K, _p(x0), _p(gl), _p(self.inputs["off"]), 0, _p(X), _p(U), self.q) == 0
        self.sync()
        return dict(obst=obst.cpu().numpy(), state=state.cpu().numpy().view(np.uint32), X=X.cpu().numpy().reshape(c, K, self.N + 1, 5),
                    U=U.cpu().numpy().reshape(c, K, self.N, 2))


def check_call(rig, pre, post, want, assign, ref, inputs0):
    """one call's arrays `post` against the restatement `want` of the state `pre`, and a started group against the existing entry points.  Returns the largest
    difference seen among the seeded rows of X."""
    G, K = rig.G, rig.K
    assert rig.bd.intact()
    for n, a in rig.inputs_host().items():
        assert np.array_equal(a, inputs0[n]), f"{n} is an input"
    started = np.repeat(np.asarray(assign) >= 0, K)
    for n in sc.ARRAYS:
        if n == "X":                                              # the seeded rows are computed values; every other row is exact
            assert np.array_equal(post[n][~started], want[n][~started]), n
            assert np.array_equal(post[n][~started], pre[n][~started]), n
        else:
            assert np.array_equal(post[n], want[n], equal_nan=True), (n, post[n], want[n])
    worst = 0.0
    for g in np.nonzero(np.asarray(assign) >= 0)[0]:
        k, rows = int(assign[g]), slice(g * K, (g + 1) * K)
        assert np.array_equal(post["obst"][g], ref["obst"][k]) and np.array_equal(post["state"][g], ref["state"][k]), (g, k)      # bit for bit
        assert np.array_equal(post["X"][rows][:, 0], ref["X"][k][:, 0]) and np.array_equal(post["X"][rows][:, 0], np.tile(post["x"][g], (K, 1)))
        assert np.array_equal(post["U"][rows], ref["U"][k]) and not post["U"][rows].any()
        d = max(np.abs(post["X"][rows] - ref["X"][k]).max(), np.abs(post["X"][rows] - want["X"][rows]).max())
        assert d <= TOL, (g, k, d)
        worst = max(worst, d)
        for m in range(K):                                        # the member inputs are the group's rows
            assert np.array_equal(post["member_x"][g * K + m], post["x"][g]) and np.array_equal(post["member_obst"][g * K + m], post["obst"][g])
            assert np.array_equal(post["member_goal"][g * K + m], post["goal"][g]) and post["member_flags"][g * K + m] == 0
    for g in np.nonzero(np.asarray(assign) == sc.KEEP)[0]:        # kept: every word of the group and of its members, bit for bit
        for n, (r, _, _) in sc.ARRAYS.items():
            if r in ("G", "B"):
                sel = slice(g * K, (g + 1) * K) if r == "B" else g
                assert np.array_equal(post[n][sel], pre[n][sel], equal_nan=True), (n, g)
    return worst


# ---------------------------------------------------------------------------------------------------------------- 1. the C ABI against the restatement
SHAPES = [(2, 1, 1, 3), (20, 5, 3, 5), (62, 10, 2, 3), (31, 12, 3, 2), (20, 3, 64, 1)]
SHAPE_IDS = ["N%d-no%d-K%d-G%d" % s for s in SHAPES]
SHAPE_SCENARIO = {(62, 10, 2, 3): "EDGE", (31, 12, 3, 2): "CENTER"}
ONE_ROW = (31, 12, 3, 2)             # this shape starts every seed from one start and goal row (per_seed = 0)


def _progress(a, roles, rng):
    """the arrays of groups that have run for a while: bookkeeping, states and iterates that are no longer those of a start; a group ends by its role"""
    G = len(roles)
    a = {n: v.copy() for n, v in a.items()}
    a["ep_steps"][:] = rng.integers(1, MAX_STEPS - 1, G); a["lost"][:] = rng.integers(0, 3, G); a["switched"][:] = rng.integers(0, 4, G)
    a["min_margin"][:] = rng.uniform(-0.5, 3.0, G)
    for n in ("x", "obst", "X", "U", "member_x", "member_obst"):
        a[n] = a[n] + rng.uniform(-0.5, 0.5, a[n].shape)
    for g, role in enumerate(roles):
        if role == "flag":
            a["ep_flags"][g] = 1 | (4 if g % 8 == 0 else 0)
        elif role == "budget":
            a["ep_steps"][g] = MAX_STEPS
        else:
            a["ep_flags"][g] = 2 * (g % 2)                        # a running group may have left the arena: bit 0 alone ends an episode
    return a


def _abi_sequence(mg, shape):
    import torch
    mpc_gpu, _ = mg
    from mpc_gpu import world
    N, no, K, G = shape
    roles = [("flag", "keep", "budget", "keep")[g % 4] for g in range(G)]
    nfin = sum(r != "keep" for r in roles)
    count = G + max(nfin - 1, 1)                                  # two or more finished: the last of them finds no seed left
    rng = np.random.default_rng(100 * N + K)
    start, goal_rows = sc_rows(count, rng)
    if shape == ONE_ROW:
        start, goal_rows = start[:1], goal_rows[:1]
    offsets = np.linspace(-5.0, 5.0, K) if K > 5 else ec.OFFSETS[K]
    worst = 0.0
    with make(mpc_gpu, N, no, count * K) as s:
        rig = Rig(mpc_gpu, torch, s, G, K, count, offsets, start, goal_rows, SHAPE_SCENARIO.get(shape, "RANDOM"))
        ref, inputs0 = rig.references(), rig.inputs_host()
        # the first call, from the preset state: every group is filled
        pre = rig.snapshot()
        want, assign = rig.model(world, pre)
        assert rig.call() == 0, rig.L.mpc_last_error()
        post = rig.snapshot()
        assert assign.tolist() == list(range(G)) and post["cursor"].tolist() == [G, G] and np.isnan(post["res_f"]).all()
        worst = max(worst, check_call(rig, pre, post, want, assign, ref, inputs0))
        # nothing finished: nothing is written
        assert rig.call() == 0
        same = rig.snapshot()
        for n in sc.ARRAYS:
            assert np.array_equal(same[n], post[n], equal_nan=True), n
        # kept, finished by the flag, finished by the budget, drained
        pre = _progress(same, roles, rng)
        rig.put(pre)
        want, assign = rig.model(world, pre)
        assert rig.call() == 0
        post = rig.snapshot()
        fin = [g for g, r in enumerate(roles) if r != "keep"]
        assert [assign[g] for g in fin[:count - G]] == list(range(G, count)) and all(assign[g] == sc.DRAIN for g in fin[count - G:])
        assert (nfin < 2) or (assign == sc.DRAIN).sum() == 1
        assert all(assign[g] == sc.KEEP for g, r in enumerate(roles) if r == "keep") and post["cursor"].tolist() == [count, G - (nfin - (count - G))]
        worst = max(worst, check_call(rig, pre, post, want, assign, ref, inputs0))
        # every running group ends on its budget: all parked, all drained
        pre = {n: v.copy() for n, v in post.items()}
        pre["ep_steps"][pre["slot_seed"] >= 0] = MAX_STEPS
        rig.put(pre)
        want, assign = rig.model(world, pre)
        assert rig.call() == 0
        post = rig.snapshot()
        assert (assign == sc.DRAIN).all() and post["cursor"].tolist() == [count, 0] and (post["slot_seed"] == -1).all() and (post["member_flags"] == 1).all()
        assert (post["res_i"][:, 0] >= 0).all() and not np.isnan(post["res_f"]).any() and (post["ep_flags"] & 1).all()
        check_call(rig, pre, post, want, assign, ref, inputs0)
    print(f"MULTISTART-SWEEP refill {shape}: roles {roles}, {count} seeds; largest |X - mpc_seed_guesses_dev| and |X - numpy| over the seeded rows {worst:.3e}")


def sc_rows(count, rng):
    """`count` distinct start and goal rows inside the arena, the start with a speed and a turn rate of its own"""
    start = np.column_stack([rng.uniform(-7.0, -3.0, count), rng.uniform(-7.0, -3.0, count), rng.uniform(0.2, 1.3, count), rng.uniform(0.0, 0.5, count),
                             rng.uniform(-0.2, 0.2, count)])
    return start, np.column_stack([rng.uniform(3.0, 7.0, count), rng.uniform(3.0, 7.0, count)])


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_the_refill_against_the_restatement(mg, shape):
    on_own_stream(_abi_sequence, mg, shape)


# ---------------------------------------------------------------------------------------------------------------- 2. further C-ABI cases
def _more_groups_than_seeds(mg):
    import torch
    mpc_gpu, _ = mg
    from mpc_gpu import world
    N, no, K, G, count = 8, 2, 3, 6, 2
    rng = np.random.default_rng(3)
    start, goal_rows = sc_rows(count, rng)
    with make(mpc_gpu, N, no, G * K) as s:
        rig = Rig(mpc_gpu, torch, s, G, K, count, ec.OFFSETS[K], start, goal_rows)
        ref, inputs0 = rig.references(), rig.inputs_host()
        pre = rig.snapshot()
        want, assign = rig.model(world, pre)
        assert rig.call() == 0
        post = rig.snapshot()
        assert assign.tolist() == [0, 1] + [sc.DRAIN] * 4 and post["cursor"].tolist() == [2, 2] and post["slot_seed"].tolist() == [0, 1, -1, -1, -1, -1]
        check_call(rig, pre, post, want, assign, ref, inputs0)
        for n in ("x", "obst", "goal", "X", "U", "state", "member_x", "member_obst", "member_goal"):      # a group that never held a seed is drained, not touched
            rows = slice(2 * K, None) if sc.ARRAYS[n][0] == "B" else slice(2, None)
            assert np.array_equal(post[n][rows], pre[n][rows]), n


def test_more_group_slots_than_seeds(mg):
    on_own_stream(_more_groups_than_seeds, mg)


def _refusals(mg):
    import torch
    mpc_gpu, _ = mg
    from mpc_gpu import world
    ERR = mpc_gpu._lib.MPC_ERR_ARG
    N, no, K, G, count = 5, 2, 3, 2, 3
    start, goal_rows = sc_rows(count, np.random.default_rng(4))
    with make(mpc_gpu, N, no, count * K) as s:
        rig = Rig(mpc_gpu, torch, s, G, K, count, ec.OFFSETS[K], start, goal_rows)
        assert rig.call() == 0
        pre, inputs0 = rig.snapshot(), rig.inputs_host()
        A = mpc_gpu._lib.GroupRefillArrays
        fields = {n: getattr(rig.arr, n) for n, _ in A._fields_}
        cases = [(dict(h=None), b"null handle"), (dict(K=0), b"K must be"), (dict(K=65), b"K must be"), (dict(G=0), b"groups"), (dict(G=-1), b"groups"),
                 (dict(G=4), b"max_batch"), (dict(count=-1), b"seed_count"), (dict(max_steps=0), b"max_steps"), (dict(scenario=3), b"scenario"),
                 (dict(scenario=-1), b"scenario"), (dict(per_seed=2), b"per_seed"), (dict(per_seed=-1), b"per_seed")] \
            + [({n: None}, b"null") for n in ("box", "start", "goal_rows", "off", "arr")] \
            + [(dict(arr=A(**{k: v for k, v in fields.items() if k != n})), b"null") for n in fields]
        for kw, word in cases:
            assert rig.call(**kw) == ERR and word in rig.L.mpc_last_error(), (kw, rig.L.mpc_last_error())
        # not offered for groups: refused, not ignored
        i32 = lambda *sh: torch.zeros(*sh, dtype=torch.int32, device=_dev(torch))
        f64 = lambda *sh: torch.zeros(*sh, dtype=torch.float64, device=_dev(torch))
        log, res_log = i32(G, 4), i32(count, 3)
        s.set_refill_tables_dev(log=log, res_log=res_log)
        assert rig.call() == ERR and b"not offered for groups" in rig.L.mpc_last_error()
        s.set_refill_tables_dev()
        ring = dict(ring_state=i32(4, sc.STATE_WORDS), ring_obst=f64(4, no, 4), ring_tag=i32(4) - 1)
        s.episode_ring_dev(4, **ring)
        assert rig.call() == ERR and b"not offered for groups" in rig.L.mpc_last_error()
        s.episode_ring_dev(0)
        T = 4
        trace = dict(seed_row=i32(count), slot_state=i32(G, 2), len=i32(1), x=f64(1, T + 1, 5), obst=f64(1, T + 1, no, 4), u=f64(1, T, 2), status=i32(1, T), iters=i32(1, T))
        s.episode_trace_set_dev(1, T, **trace)
        assert rig.call() == ERR and b"not offered for groups" in rig.L.mpc_last_error()
        s.episode_trace_set_dev(0)
        post = rig.snapshot()
        for n in pre:
            assert np.array_equal(pre[n], post[n], equal_nan=True), n                             # nothing was launched
        assert rig.bd.intact() and all(np.array_equal(a, inputs0[n]) for n, a in rig.inputs_host().items())
        # ... and with everything detached again the call is taken: nothing has finished, nothing is written
        assert rig.call() == 0 and all(np.array_equal(pre[n], v, equal_nan=True) for n, v in rig.snapshot().items())
        want, assign = rig.model(world, sc.first_call(G, K, count, N, no))
        assert np.array_equal(pre["slot_seed"], want["slot_seed"]) and np.array_equal(pre["obst"], want["obst"])


def test_refusals_leave_every_array_unchanged(mg):
    on_own_stream(_refusals, mg)


# ---------------------------------------------------------------------------------------------------------------- 3. the sweep against the batch
_BATCH = {}


def _problem():
    d = sc.SWEEP
    return dict(offsets=ec.OFFSETS[d["K"]], incumbent_margin=d["margin"], N=d["N"], Tf=d["Tf"], n_obst=d["no"], max_iter=d["max_iter"])


def batch(mpc_gpu, select_by):
    """the yardstick: run_multistart_episodes on one batch of the scene's 9 groups; computed once per selection rule, returned read-only"""
    if select_by not in _BATCH:
        d = sc.SWEEP
        r = mpc_gpu.run_multistart_episodes(sc.START, sc.GOAL, d["scenario"], first_seed=d["first_seed"], select_by=select_by, **_problem())
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _BATCH[select_by] = r
    return _BATCH[select_by]


def sweep(mpc_gpu, slots, select_by, **kw):
    d = sc.SWEEP
    return mpc_gpu.run_multistart_sweep(sc.START, sc.GOAL, d["scenario"], (d["first_seed"], d["count"]), slots, select_by=select_by, poll_every=1, **_problem(), **kw)


def against_the_batch(tag, r, ref, slots):
    from mpc_gpu.episodes import refill_schedule
    d = sc.SWEEP
    lengths = (ref["table"][:, 4] + ref["table"][:, 1]).astype(np.int64)
    close = lambda a, b: float(np.abs(np.where(a == b, 0.0, a - b)).max())
    print(f"MULTISTART-SWEEP {tag}: lengths {lengths.tolist()} steps_run {r['steps_run']} solves {r['solves']} lost {r['lost_steps'].tolist()} switched "
          f"{r['switched_steps'].tolist()}; largest |sweep - batch| table {close(r['table'], ref['table']):.3e} x_last {close(r['x_last'], ref['x_last']):.3e}")
    assert r["table"].shape == (d["count"], 6) and r["x_last"].shape == (d["count"], 5)
    assert np.array_equal(r["table"][:, [0, 1, 4, 5]], ref["table"][:, [0, 1, 4, 5]])             # flags and step counts
    assert np.array_equal(r["lost_steps"], ref["lost_steps"]) and np.array_equal(r["switched_steps"], ref["switched_steps"])
    assert close(r["table"], ref["table"]) <= 1e-9 and close(r["x_last"], ref["x_last"]) <= 1e-9
    assert r["solves"] == d["K"] * int(r["table"][:, 4].sum() + r["table"][:, 1].sum()) == ref["solves"]
    want = refill_schedule(lengths, slots)
    assert np.array_equal(r["schedule"][:, 0], want["slot"]) and np.array_equal(r["schedule"][:, 1], want["start"]) and r["steps_run"] == want["steps"]
    assert r["steps_run"] < d["max_iter"] * -(-d["count"] // slots)


def _sweep_against_batch(mg, slots, select_by):
    mpc_gpu, _ = mg
    ref = batch(mpc_gpu, select_by)
    r1, r2 = sweep(mpc_gpu, slots, select_by), sweep(mpc_gpu, slots, select_by)
    against_the_batch(f"{slots} slots by {select_by}", r1, ref, slots)
    for k in r1:
        assert np.array_equal(r1[k], r2[k], equal_nan=True), k                                   # a second run gives the same bits
    lengths = ref["table"][:, 4] + ref["table"][:, 1]
    assert len(set(lengths.tolist())) >= 3 and (ref["table"][:, 1] == 1).any() and (ref["table"][:, 1] == 0).any()      # what the host test found on the oracle


@pytest.mark.parametrize("slots, select_by", [(4, "cost"), (2, "rollout")])
def test_the_sweep_against_the_batch(mg, slots, select_by):
    on_own_stream(_sweep_against_batch, mg, slots, select_by)


def _callers_solver(mg):
    mpc_gpu, _ = mg
    d = sc.SWEEP
    ref = batch(mpc_gpu, "cost")
    with mpc_gpu.MultiStartMpc(d["N"], d["no"], d["Tf"], scenarios=4, offsets=ec.OFFSETS[d["K"]], incumbent_margin=d["margin"]) as ms:
        name0 = ms.inner.kernel_name(ms.B)
        r_sqp = sweep(mpc_gpu, 4, "cost", solver=ms, sqp=(2, 0.0))
        assert ms.inner.kernel_name(ms.B) == name0 and not ms.inner._sqp_on and not (ms._warm or ms._fused_warm)      # SQP off again, the loop forgotten
        assert r_sqp["table"].shape == (d["count"], 6) and not np.array_equal(r_sqp["x_last"], ref["x_last"])           # (it did run two iterations per step)
        against_the_batch("4 slots on a caller's handle", sweep(mpc_gpu, 4, "cost", solver=ms), ref, 4)
        with pytest.raises(ValueError, match="group slots"):
            sweep(mpc_gpu, 2, "cost", solver=ms)


def test_a_callers_solver_leaves_as_it_came(mg):
    on_own_stream(_callers_solver, mg)
