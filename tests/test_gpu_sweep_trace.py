"""Per-seed closed-loop trajectories of a seed sweep, recorded on the device (mpc_episode_trace_set_dev / mpc_episode_trace_dev, run_seed_sweep(trace=)).

The yardstick is the path that exists without the feature: trace_cases.batch_trace runs run_episodes' own loop on ONE batch that holds every seed and clones
the arrays behind each step (and holds itself to run_episodes(record=True) bit for bit).  Both mappings give an instance a wavefront to itself, so a traced
seed's rows equal its column of that batch EXACTLY (np.array_equal), whatever slot and control step it ran at.  Sizes are the smallest at which a trace can
go wrong: more seeds than slots, an offset first seed, a count that is no multiple of the slots, a subset of the seeds, episodes that end by budget."""
import numpy as np
import pytest

import sweep_cases as sc
import sweep_feature_cases as fc
import trace_cases as tc
from test_gpu_sweep import mapping, sweep  # noqa: F401  (the fixture: both lane mappings, restored behind every test)

pytestmark = pytest.mark.gpu

SEEDS, SLOTS = (37, 10), 3          # an offset first seed, a count that is no multiple of the slots
BUDGET = 80                         # control steps at which, on the yardstick, some seeds of 37 .. 46 have reached the goal (the shortest take 36 .. 57) and
#                                     the others have not (the longest take over 200): test_budget_end asserts both kinds on the yardstick itself


@pytest.fixture
def mg(built):
    import mpc_gpu
    mpc_gpu.BatchedMpc.default_lanes_per_stage = 0
    return mpc_gpu


_FULL = {}


def full_trace(mg):
    """case 1's sweep, shared with the cases that compare against it"""
    key = mg.BatchedMpc.default_lanes_per_stage
    if key not in _FULL:
        _FULL[key] = sweep(mg, "RANDOM", SEEDS, SLOTS, trace=True)
    return _FULL[key]


def assert_same_trace(a, b):
    assert sorted(a) == sorted(b)
    for n in a:
        assert a[n].dtype == b[n].dtype and np.array_equal(a[n], b[n]), n


def test_all_seeds_traced(mapping):
    bt = tc.batch_trace(mapping, *SEEDS)
    r = full_trace(mapping)
    plain = sweep(mapping, "RANDOM", SEEDS, SLOTS)
    assert sorted(r["trace"]) == list(range(10))
    print("episode lengths", bt["lengths"].tolist())
    assert len(set(bt["lengths"].tolist())) > 3, "the yardstick itself: episodes of unequal length"
    for k in range(10):
        tc.assert_trace_is_column(r["trace"][k], bt, k)
    for ref in (plain, bt):
        assert np.array_equal(r["table"], ref["table"]) and np.array_equal(r["x_last"], ref["x_last"])
    assert r["solves"] == plain["solves"] == int(bt["lengths"].sum())


def test_budget_end(mapping):
    bt = tc.batch_trace(mapping, *SEEDS, max_iter=BUDGET)
    by_budget = np.nonzero((bt["table"][:, 1] == 0) & (bt["table"][:, 4] == BUDGET))[0]
    by_goal = np.nonzero(bt["table"][:, 1] == 1)[0]
    print("ended by budget", by_budget.tolist(), "by reaching the goal", by_goal.tolist())
    assert by_budget.size >= 1 and by_goal.size >= 1 and by_budget.size + by_goal.size == 10, "the yardstick itself shows both kinds of end"
    r = sweep(mapping, "RANDOM", SEEDS, SLOTS, max_iter=BUDGET, trace=True)
    assert np.array_equal(r["table"], bt["table"]) and np.array_equal(r["x_last"], bt["x_last"])
    for k in range(10):
        tc.assert_trace_is_column(r["trace"][k], bt, k)
    for k in by_budget:
        t = r["trace"][int(k)]
        assert t["u"].shape[0] == BUDGET and t["simX"].shape[0] == BUDGET + 1
        assert t["simX"][BUDGET].any() and t["obst_traj"][BUDGET].any() and t["pred"][BUDGET - 1].any()       # row L is filled (the arrays start as zeros)
        assert np.array_equal(t["simX"][BUDGET], r["x_last"][k])
    for k in by_goal:
        assert r["trace"][int(k)]["u"].shape[0] < BUDGET and np.array_equal(r["trace"][int(k)]["simX"][-1], r["x_last"][k])


def test_subset(mapping):
    full = full_trace(mapping)
    with mapping.BatchedMpc(max_batch=SLOTS, **sc.PROBLEM) as m:
        r = mapping.run_seed_sweep(sc.START, sc.GOAL, "RANDOM", SEEDS, SLOTS, solver=m, trace=[0, 4, 9])
        shapes = dict(m.trace_shapes)
    assert sorted(r["trace"]) == [0, 4, 9]
    for k in (0, 4, 9):
        assert_same_trace(r["trace"][k], full["trace"][k])
    assert np.array_equal(r["table"], full["table"]) and np.array_equal(r["x_last"], full["x_last"])          # (full's table is the untraced one: case 1)
    N, no, T = sc.PROBLEM["N"], sc.PROBLEM["n_obst"], 400
    assert shapes == dict(seed_row=(10,), slot_state=(SLOTS, 2), len=(3,), x=(3, T + 1, 5), obst=(3, T + 1, no, 4), u=(3, T, 2), status=(3, T), iters=(3, T),
                          pred=(3, T, N + 1, 5))
    other = sweep(mapping, "RANDOM", SEEDS, SLOTS, trace=(9, 4))            # the order given is the order of the rows, not of the result
    assert sorted(other["trace"]) == [4, 9]
    for k in (4, 9):
        assert_same_trace(other["trace"][k], full["trace"][k])


@pytest.mark.parametrize("qp", ["problem", "low-qp"])
def test_with_the_other_sweep_features(mapping, qp):
    """status log, ring and per-seed radii together with a trace; low-qp (8 interior-point iterations, 80 control steps) is the problem on which the status words
    are not all zero"""
    problem, kw = (sc.PROBLEM, {}) if qp == "problem" else (dict(sc.PROBLEM, qp_iter_max=8), dict(max_iter=80))
    r_safe = fc.arrays(10)["r_safe"]
    feat = dict(status_log=True, ring=4, r_safe=r_safe, problem=problem, **kw)
    r = sweep(mapping, "RANDOM", SEEDS, SLOTS, trace=True, **feat)
    plain = sweep(mapping, "RANDOM", SEEDS, SLOTS, **feat)
    assert np.array_equal(r["table"], plain["table"]) and np.array_equal(r["x_last"], plain["x_last"])
    for n in ("status2", "status4", "first_bad"):
        assert np.array_equal(r[n], plain[n]), n
    bad_steps = 0
    for k in range(10):
        st = r["trace"][k]["status"]
        assert r["status2"][k] == (st == 2).sum() and r["status4"][k] == (st == 4).sum(), k
        nz = np.nonzero(st)[0]
        assert r["first_bad"][k] == (nz[0] if nz.size else -1), k
        bad_steps += nz.size
    print(qp, "control steps with a status != 0:", bad_steps)
    if qp == "low-qp":
        assert bad_steps > 0, "the case itself: some solve ends with a status != 0"
    bt = tc.batch_trace(mapping, *SEEDS, problem=problem, r_safe=r_safe, **kw)
    assert np.array_equal(r["table"], bt["table"])
    for k in range(10):
        tc.assert_trace_is_column(r["trace"][k], bt, k)


def test_without_pred(mapping):
    full = full_trace(mapping)
    r = sweep(mapping, "RANDOM", SEEDS, SLOTS, trace=True, trace_pred=False)
    assert np.array_equal(r["table"], full["table"])
    for k in range(10):
        assert "pred" not in r["trace"][k]
        assert_same_trace(r["trace"][k], {n: a for n, a in full["trace"][k].items() if n != "pred"})
    with pytest.raises(ValueError, match="trace_pred=False"):
        mapping.sweep_record(r, 4)
    v = mapping.visualisation_inputs(mapping.sweep_record(full, 4), 0)      # ... and with them, the record is the reference's visualisation input
    L = full["trace"][4]["u"].shape[0]
    assert v["trajectory"].shape == (2, L + 1) and v["pred"].shape == (L + 1, 21, 2) and len(v["obstacles"]) == 5


def test_fifteen_obstacles(mg):
    """N 10, 15 obstacles: the multi-wavefront solve kernel (which has the one mapping, two lanes per stage) and an obstacle row of 60 doubles; 6 seeds
    through 2 slots"""
    mapping = mg
    with mapping.BatchedMpc(max_batch=2, **sc.WIDE_PROBLEM) as probe:
        assert "rti_wide_kernel" in probe.kernel_name(2)
    bt = tc.batch_trace(mapping, 0, 6, problem=sc.WIDE_PROBLEM, max_iter=60)
    r = sweep(mapping, "RANDOM", (0, 6), 2, problem=sc.WIDE_PROBLEM, max_iter=60, trace=True)
    plain = sweep(mapping, "RANDOM", (0, 6), 2, problem=sc.WIDE_PROBLEM, max_iter=60)
    for ref in (plain, bt):
        assert np.array_equal(r["table"], ref["table"]) and np.array_equal(r["x_last"], ref["x_last"])
    for k in range(6):
        assert r["trace"][k]["obst_traj"].shape[1:] == (15, 4) and r["trace"][k]["pred"].shape[1:] == (11, 5)
        tc.assert_trace_is_column(r["trace"][k], bt, k)


def test_a_callers_solver_leaves_as_it_came(mapping):
    import torch
    from mpc_gpu import _lib
    full = full_trace(mapping)
    with mapping.BatchedMpc(max_batch=4, **sc.PROBLEM) as m:
        traced = mapping.run_seed_sweep(sc.START, sc.GOAL, "RANDOM", SEEDS, SLOTS, solver=m, trace=[2, 7])
        again = mapping.run_seed_sweep(sc.START, sc.GOAL, "RANDOM", SEEDS, SLOTS, solver=m)
        dev = torch.device("cuda", 0)
        z = torch.zeros(4, 5 * 4, dtype=torch.float64, device=dev); w = torch.zeros(4, dtype=torch.int32, device=dev)
        with pytest.raises(_lib.MpcError, match="no trace attached"):          # detached: the entry point refuses, and launches nothing
            m.episode_trace_dev(3, _lib.TRACE_START, w, z, z, ep_flags=w, ep_steps=w)
        torch.cuda.synchronize()
    assert "trace" not in again and sorted(traced["trace"]) == [2, 7]
    assert np.array_equal(again["table"], full["table"]) and np.array_equal(again["x_last"], full["x_last"])
    assert np.array_equal(traced["table"], full["table"])
    for k in (2, 7):
        assert_same_trace(traced["trace"][k], full["trace"][k])


def refuse(*a, **kw):
    """stands in for a binding whose library call is refused: a Python exception, nothing is launched"""
    from mpc_gpu import _lib
    raise _lib.MpcError("injected refusal")


def assert_detached(m, name0, batch):
    """the handle runs the kernel it came with, and holds no trace"""
    import torch
    from mpc_gpu import _lib
    assert m.kernel_name(batch) == name0
    dev = torch.device("cuda", 0)
    z = torch.zeros(4, 5 * 4, dtype=torch.float64, device=dev); w = torch.zeros(4, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.MpcError, match="no trace attached"):
        m.episode_trace_dev(3, _lib.TRACE_START, w, z, z, ep_flags=w, ep_steps=w)
    torch.cuda.synchronize()


@pytest.mark.parametrize("fails_at", ["episode_trace_set_dev", "set_refill_tables_dev"])
def test_a_failed_attach_leaves_a_callers_solver_as_it_came(mapping, fails_at):
    """every feature of a sweep on a caller's handle, and the attach named fails (in Python, before any launch): the handle is at level 0 again, nothing is
    attached, and the next plain sweep on it gives the batch harness's rows"""
    from mpc_gpu import _lib
    ref = sc.batch_reference(mapping, "RANDOM", *SEEDS)
    f = fc.arrays(10)
    during = []
    with mapping.BatchedMpc(max_batch=4, **sc.PROBLEM) as m:
        name0 = m.kernel_name(3)
        setattr(m, fails_at, lambda *a, **kw: (during.append(m.kernel_name(3)), refuse())[1])
        with pytest.raises(_lib.MpcError, match="injected refusal"):
            mapping.run_seed_sweep(sc.START, sc.GOAL, "RANDOM", SEEDS, SLOTS, solver=m, r_safe=f["r_safe"], active=f["active"], bounds=f["bounds"],
                                   status_log=True, ring=2, trace=[2, 7])
        delattr(m, fails_at)                        # (the handle's own binding again)
        assert len(during) == 1 and during[0] != name0, "the case itself: the features were on when the attach failed"
        assert_detached(m, name0, 3)
        again = mapping.run_seed_sweep(sc.START, sc.GOAL, "RANDOM", SEEDS, SLOTS, solver=m)
    assert np.array_equal(again["table"], ref["table"]) and np.array_equal(again["x_last"], ref["x_last"])


def test_a_failed_step_leaves_run_episodes_callers_solver_as_it_came(mapping):
    """run_episodes with radii and bounds on a caller's handle, and the second fused step fails (in Python): level 0 again, and the next plain call on the
    handle gives the reference table"""
    from mpc_gpu import _lib
    ref = sc.batch_reference(mapping, "RANDOM", *SEEDS)
    f = fc.arrays(10)
    x0, goal = np.tile(sc.START, (10, 1)), np.tile(sc.GOAL, (10, 1))
    kw = dict(first_seed=SEEDS[0], compact_from=None, N=sc.PROBLEM["N"], Tf=sc.PROBLEM["Tf"], n_obst=sc.PROBLEM["n_obst"])
    during = []
    with mapping.BatchedMpc(max_batch=10, **sc.PROBLEM) as m:
        name0 = m.kernel_name(10)
        step = m.closed_loop_step_dev
        m.closed_loop_step_dev = lambda *a, **k: refuse() if during else (during.append(m.kernel_name(10)), step(*a, **k))[1]
        with pytest.raises(_lib.MpcError, match="injected refusal"):
            mapping.run_episodes(x0, goal, "RANDOM", solver=m, r_safe=f["r_safe"], bounds=f["bounds"], **kw)
        del m.closed_loop_step_dev
        assert len(during) == 1 and during[0] != name0, "the case itself: the features were on when the step failed"
        assert_detached(m, name0, 10)
        again = mapping.run_episodes(x0, goal, "RANDOM", solver=m, **kw)
    assert np.array_equal(again["table"], ref["table"]) and np.array_equal(again["x_last"], ref["x_last"])


@pytest.mark.parametrize("driver", ["run_seed_sweep", "run_episodes"])
def test_own_handles_are_closed_on_failure(mapping, monkeypatch, driver):
    """the same failures without solver=: the handle the driver made is closed, once, before the exception leaves the call"""
    from mpc_gpu import _lib
    f = fc.arrays(10)
    if driver == "run_episodes":
        with mapping.BatchedMpc(max_batch=10, **sc.PROBLEM) as g:            # (explicit obstacle states: the driver then makes ONE handle, its own)
            obst = g.generate_scenarios("RANDOM", 10, seed0=SEEDS[0])
    closed, stepped = [], []
    close, step = mapping.BatchedMpc.close, mapping.BatchedMpc.closed_loop_step_dev

    def counting_close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            closed.append(id(self))
        close(self)
    monkeypatch.setattr(mapping.BatchedMpc, "close", counting_close)
    with pytest.raises(_lib.MpcError, match="injected refusal") as e:
        if driver == "run_seed_sweep":
            monkeypatch.setattr(mapping.BatchedMpc, "episode_trace_set_dev", refuse)
            sweep(mapping, "RANDOM", SEEDS, SLOTS, r_safe=f["r_safe"], status_log=True, ring=2, trace=[2, 7])
        else:
            monkeypatch.setattr(mapping.BatchedMpc, "closed_loop_step_dev", lambda self, *a, **k: refuse() if stepped else (stepped.append(1), step(self, *a, **k))[1])
            mapping.run_episodes(np.tile(sc.START, (10, 1)), np.tile(sc.GOAL, (10, 1)), obst, r_safe=f["r_safe"], bounds=f["bounds"], random_move=False, **sc.PROBLEM)
    assert len(closed) == 1          # (`e` still holds the call's frames, and with them the handle: it was closed by the driver, not by the collector)
    del e


def test_argument_refusals_and_a_skipped_start_through_the_c_abi(mapping):
    """MPC_ERR_ARG naming the field with nothing launched; then the protocol itself on two slots: a seed whose START launch was skipped shows len = -1 and not
    a wrong row 0, and the other rows are untouched"""
    import torch
    from mpc_gpu import _lib
    from test_gpu_sweep import STEP_FLAGS
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    with mapping.BatchedMpc(max_batch=2, **sc.PROBLEM) as m:
        arr = sc.SlotArrays(sc.Plain(torch, dev), m, 2, 4, L.mpc_noise_state_words())
        alloc = sc.Plain(torch, dev)
        T = 6
        t = dict(seed_row=alloc.i32(4), slot_state=alloc.i32(2, 2), len=alloc.i32(2, init=-7), x=alloc.f64(2, T + 1, 5, init=-7.0), obst=alloc.f64(2, T + 1, 5, 4, init=-7.0),
                 u=alloc.f64(2, T, 2, init=-7.0), status=alloc.i32(2, T, init=-7), iters=alloc.i32(2, T, init=-7), pred=alloc.f64(2, T, 21, 5, init=-7.0))
        t["seed_row"].copy_(torch.tensor([1, 0, -1, -1], dtype=torch.int32)); t["slot_state"].copy_(torch.tensor([[-1, 0], [-1, 0]], dtype=torch.int32))
        u0 = alloc.f64(2, 2)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        s = stream.cuda_stream
        step_args = (arr.slot_seed, arr.x0, arr.obst, arr.X, u0, arr.status, arr.iters, arr.flags, arr.steps)
        with pytest.raises(_lib.MpcError, match="no trace attached"):
            m.episode_trace_dev(2, _lib.TRACE_STEP, *step_args, stream=s)
        for kw, word in ((dict(rows=-1), "rows"), (dict(max_steps=0), "max_steps"), (dict(seed_row=None), "seed_row"), (dict(slot_state=None), "slot_state"),
                         (dict(len=None), "len"), (dict(x=None), "x is null"), (dict(obst=None), "obst"), (dict(u=None), "u is null"), (dict(status=None), "status"),
                         (dict(iters=None), "iters")):
            with pytest.raises(_lib.MpcError, match=word):
                m.episode_trace_set_dev(**dict(dict(rows=2, max_steps=T, **t), **kw))
        with pytest.raises(_lib.MpcError, match="no trace attached"):              # a refused attach attaches nothing
            m.episode_trace_dev(2, _lib.TRACE_START, *step_args, stream=s)
        m.episode_trace_set_dev(2, T, **t)
        for a, word in (((3, 0) + step_args, "slots"), ((0, 0) + step_args, "slots"), ((2, 2) + step_args, "phase"), ((2, -1) + step_args, "phase"),
                        ((2, 1) + step_args[:4] + (None,) + step_args[5:], "u0"), ((2, 1) + step_args[:5] + (None,) + step_args[6:], "status"),
                        ((2, 1) + step_args[:3] + (None,) + step_args[4:], "X"), ((2, 0, None) + step_args[1:], "slot_seed"), ((2, 0) + step_args[:7] + (None, arr.steps), "ep_flags")):
            with pytest.raises(_lib.MpcError, match=word):
                m.episode_trace_dev(*a, stream=s)
        torch.cuda.synchronize()
        assert (t["len"].cpu().numpy() == -7).all() and (t["x"].cpu().numpy() == -7.0).all() and t["slot_state"].cpu().tolist() == [[-1, 0], [-1, 0]]
        # the protocol on seeds 0 and 1 (rows 1 and 0); the START launch of the first control step is skipped
        rf = _lib.REFILL_ALIAS_BUG | _lib.REFILL_DRAW_NOISE
        with torch.cuda.stream(stream):
            arr.refill(m, "RANDOM", 0, T, rf, s)
            x_start = arr.x0.clone()
            m.closed_loop_step_dev(2, arr.x0, arr.obst, arr.goal, arr.X, arr.U, u0, None, arr.status, arr.iters, arr.noise, flags=STEP_FLAGS, min_margin=arr.margin,
                                   ep_flags=arr.flags, ep_steps=arr.steps, stream=s)
            m.episode_trace_dev(2, _lib.TRACE_STEP, *step_args, stream=s)        # nothing started through START: STEP writes nothing
            stream.synchronize()
            assert (t["len"].cpu().numpy() == -7).all() and (t["x"].cpu().numpy() == -7.0).all()
            arr.refill(m, "RANDOM", 0, T, rf, s)
            m.episode_trace_dev(2, _lib.TRACE_START, arr.slot_seed, arr.x0, arr.obst, ep_flags=arr.flags, ep_steps=arr.steps, stream=s)      # too late: now = 1
            m.closed_loop_step_dev(2, arr.x0, arr.obst, arr.goal, arr.X, arr.U, u0, None, arr.status, arr.iters, arr.noise, flags=STEP_FLAGS, min_margin=arr.margin,
                                   ep_flags=arr.flags, ep_steps=arr.steps, stream=s)
            m.episode_trace_dev(2, _lib.TRACE_STEP, *step_args, stream=s)
            stream.synchronize()
        assert t["len"].cpu().tolist() == [-1, -1] and t["slot_state"].cpu().tolist() == [[-1, 0], [-1, 0]]
        for n in ("x", "obst", "u", "pred"):
            assert (t[n].cpu().numpy() == -7.0).all(), n
        assert (t["status"].cpu().numpy() == -7).all() and (t["iters"].cpu().numpy() == -7).all()
        assert x_start.cpu().numpy().any()
        m.episode_trace_set_dev(0)
