"""The episode drivers' shared core without a device: the lease that owns what a driver borrows on a handle (with a fake solver that records calls),
run_episodes' refusals that need no device, the one set of shape rules behind BatchedMpc's setters and run_seed_sweep's per-seed tables, and the two
loops the four drivers run on (_sweep_loop, _episode_loop) with the sweeps' shared collect (_sweep_table), driven by fakes on CPU tensors."""
import ctypes as C

import numpy as np
import pytest

from test_sweep_host import no_device  # noqa: F401  (the fixture: loading the library or creating a handle fails the test)


@pytest.fixture
def ep():
    import mpc_gpu.episodes as ep       # (pure Python: no library is loaded by the import)
    return ep


# ---------------------------------------------------------------------------------------------------------------- 1. the lease
class Boom(Exception):
    pass


class Recorder:
    """stands in for a solver and for a stream: every call is appended to `log` as (name, args); the calls listed in `fail` raise Boom(name, args)"""

    def __init__(self, log, fail=()):
        self.log, self.fail = log, fail

    def __getattr__(self, name):
        def call(*a, **kw):
            self.log.append((name, a))
            if (name, a) in self.fail:
                raise Boom(name, a)
        return call


def never():
    raise AssertionError("a caller's solver is used, none is made")


ATTACH = [("set_sqp", (3, 1e-6)), ("set_obstacle_mask", ("words",)), ("episode_ring_dev", (4,))]


def attach_three(lease):
    for name, args in ATTACH:
        lease.attach(name, *args)


def test_a_failed_apply_undoes_the_attached_features_in_reverse_order(ep):
    log = []
    m = Recorder(log, fail=[ATTACH[2]])
    with pytest.raises(Boom) as e:
        with ep._HandleLease(m, never, stream=Recorder(log)) as lease:
            assert lease.m is m
            attach_three(lease)
    assert e.value.args == ATTACH[2]
    # the third apply raised: it is not undone; the stream is synchronised in front of the first undo; a caller's solver is not closed
    assert log == ATTACH + [("synchronize", ()), ("set_obstacle_mask", (None,)), ("set_sqp", ())]


def test_an_own_handle_is_closed_exactly_once_and_last(ep):
    for fail in ([ATTACH[2]], []):
        log, made = [], []
        m = Recorder(log, fail=fail)
        try:
            with ep._HandleLease(None, lambda: made.append(1) or m) as lease:
                assert lease.m is m
                attach_three(lease)
        except Boom:
            assert fail
        assert made == [1] and [n for n, _ in log].count("close") == 1 and log[-1] == ("close", ())
        undone = [("set_obstacle_mask", (None,)), ("set_sqp", ())] if fail else [("episode_ring_dev", (0,)), ("set_obstacle_mask", (None,)), ("set_sqp", ())]
        assert log == ATTACH + undone + [("close", ())]          # (no stream given: nothing to synchronise)


def test_an_undo_that_raises_does_not_stop_the_others_and_the_first_exception_leaves(ep):
    bad_undo = ("set_obstacle_mask", (None,))
    # the block's own exception is the first
    log = []
    with pytest.raises(Boom) as e:
        with ep._HandleLease(None, lambda: Recorder(log, fail=[ATTACH[2], bad_undo]), stream=Recorder(log)) as lease:
            attach_three(lease)
    assert e.value.args == ATTACH[2]
    assert log == ATTACH + [("synchronize", ()), bad_undo, ("set_sqp", ()), ("close", ())]
    # a block that ends well: the first failing step of the exit is the one that leaves, and the steps behind it still run
    log = []
    with pytest.raises(Boom) as e:
        with ep._HandleLease(None, lambda: Recorder(log, fail=[("episode_ring_dev", (0,)), bad_undo]), stream=Recorder(log)) as lease:
            attach_three(lease)
    assert e.value.args == ("episode_ring_dev", (0,))
    assert log == ATTACH + [("synchronize", ()), ("episode_ring_dev", (0,)), bad_undo, ("set_sqp", ()), ("close", ())]
    # a stream that fails to synchronise stops nothing either
    log = []
    with pytest.raises(Boom) as e:
        with ep._HandleLease(Recorder(log), never, stream=Recorder(log, fail=[("synchronize", ())])) as lease:
            attach_three(lease)
    assert e.value.args == ("synchronize", ()) and log[-3:] == [("episode_ring_dev", (0,)), ("set_obstacle_mask", (None,)), ("set_sqp", ())]


def test_the_lease_undoes_every_setter_the_drivers_use_and_no_other(ep):
    log = []
    with ep._HandleLease(Recorder(log), never) as lease:
        for name in ep._HandleLease.OFF:
            lease.attach(name, "on")
        with pytest.raises(KeyError):
            lease.attach("set_slack_schedule", "alpha")
    off = dict(set_instance_params=(), set_obstacle_mask=(None,), set_instance_bounds=(), set_instance_bounds_dev=(None,), set_sqp=(),
               set_refill_tables_dev=(), episode_ring_dev=(0,), episode_trace_set_dev=(0,))
    assert log[8:] == [(n, off[n]) for n in reversed(list(ep._HandleLease.OFF))] and sorted(off) == sorted(ep._HandleLease.OFF)


# ---------------------------------------------------------------------------------------------------------------- 2. run_episodes refuses before the handle
class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"a refusal must not touch the caller's solver ({name})")


@pytest.mark.parametrize("solver", [None, Untouchable()], ids=["own-handle", "callers-solver"])
def test_run_episodes_refuses_before_any_setter_or_device_call(ep, no_device, solver):
    B, no = 4, 3
    x0, goal, obst = np.zeros((B, 5)), np.ones((B, 2)), np.ones((B, no, 4))
    features = dict(r_safe=np.full(B, 2.0), active=np.ones((B, no), dtype=bool), bounds=dict(bu_hi=[4.0, 4.0]), sqp=(3, 1e-6))
    run = lambda *a, **kw: ep.run_episodes(*a, solver=solver, n_obst=no, max_iter=20, **kw)
    for noise in (np.zeros((19, B, no, 2)), np.zeros((20, B, no)), np.zeros((20, B + 1, no, 2)), np.zeros((20, B, no + 1, 2))):
        with pytest.raises(ValueError, match=r"noise must be \(>= 20, 4, 3, 2\), got"):
            run(x0, goal, obst, noise=noise, **features)
    with pytest.raises(ValueError, match="pass the scenario name as `obst`"):
        run(x0, goal, obst, noise="reference", **features)
    with pytest.raises(ValueError, match="pass the scenario name as `obst`"):          # (any other word is no source either)
        run(x0, goal, "RANDOM", noise="numpy", **features)
    with pytest.raises(ValueError, match="Vary first_seed"):
        run(x0, goal, "RANDOM", seed=3, **features)
    with pytest.raises(AssertionError, match="must not touch"):          # a good call reaches the device: the fixture, behind the validation
        run(x0, goal, obst, noise=np.zeros((20, B, no, 2)), **features)


# ---------------------------------------------------------------------------------------------------------------- 3. one set of shape rules
COUNT, NO = 4, 3


def bare(monkeypatch, capture=lambda name, args: (name, args)):
    """a BatchedMpc without a handle over a library that records capture(name, args) of every call (at call time: the arrays behind the pointers die with
    the setter's frame); returns (the solver, the record)"""
    from mpc_gpu import _lib
    from mpc_gpu.solver import BatchedMpc
    calls = []

    class Lib:
        def __getattr__(self, name):
            def call(*a):
                calls.append(capture(name, a))
                return 0
            return call
    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    m = object.__new__(BatchedMpc)
    m.n_obst, m.max_batch, m._h = NO, COUNT, C.c_void_p()
    return m, calls


def at(ptr, ctype, shape):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=shape).copy()


NONE4 = dict(W=None, We=None, r_safe=None, r_hit=None)


@pytest.mark.parametrize("name,cols", [("W", 6), ("We", 4), ("r_safe", NO), ("r_hit", NO)])
def test_instance_arrays_are_normalised_alike_on_both_sides(ep, monkeypatch, name, cols):
    m, _ = bare(monkeypatch)
    radius = name.startswith("r_")
    rng = np.random.default_rng(1)
    good = [rng.uniform(0.5, 3.0, (COUNT, cols))] + ([rng.uniform(0.5, 3.0, COUNT)] if radius else [])        # radii: (rows,) too, one per instance
    for a in good + [g.tolist() for g in good]:
        batch = dict(zip(NONE4, m._instance_arrays(**dict(NONE4, **{name: a}))[0]))[name]
        sweep = ep._sweep_features(COUNT, NO, ep.DEFAULT_BOUNDS, **{name: a})[name]
        assert batch.shape == (COUNT, cols) and np.array_equal(batch, sweep)
        assert batch.dtype == sweep.dtype == np.float64 and batch.flags["C_CONTIGUOUS"] and sweep.flags["C_CONTIGUOUS"]
        assert np.array_equal(batch, np.broadcast_to(np.asarray(a, dtype=np.float64).reshape(COUNT, -1), (COUNT, cols)))
    for bad in [np.ones((COUNT, cols + 1)), np.ones((COUNT, cols, 1))] + ([] if radius else [np.ones(COUNT)]):
        with pytest.raises(ValueError, match=rf"{name} must be \(B, {cols}\)" + (r" or \(B,\)" if radius else "") + ", got"):
            m._instance_arrays(**dict(NONE4, **{name: bad}))
        with pytest.raises(ValueError, match=rf"{name} must be \(count, {cols}\)" + (r" or \(count,\)" if radius else "") + ", got"):
            ep._sweep_features(COUNT, NO, ep.DEFAULT_BOUNDS, **{name: bad})
    # the row count: each side's own rule, in its own words
    with pytest.raises(ValueError, match="the arrays before it"):
        other = {"We": np.ones((COUNT, 4))} if name == "W" else {"W": np.ones((COUNT, 6))}
        m._instance_arrays(**dict(NONE4, **other, **{name: np.ones((COUNT + 1, cols))}))
    with pytest.raises(ValueError, match=f"per-seed {name} has {COUNT + 1} rows for {COUNT} seeds"):
        ep._sweep_features(COUNT, NO, ep.DEFAULT_BOUNDS, **{name: np.ones((COUNT + 1, cols))})


def test_masks_are_normalised_alike_on_both_sides(ep, monkeypatch):
    m, calls = bare(monkeypatch, lambda fn, a: (fn, a[1], at(a[2], C.c_uint32, (a[1],))))
    active = np.array([[1, 0, 1], [0, 0, 1], [1, 1, 1], [0, 1, 0]], dtype=bool)
    for a in (active, active.tolist(), active.astype(np.int64)):
        calls.clear()
        m.set_obstacle_mask(a)
        (fn, rows, words), = calls
        assert fn == "mpc_set_obstacle_mask" and rows == COUNT
        assert np.array_equal(words, ep._sweep_features(COUNT, NO, ep.DEFAULT_BOUNDS, active=a)["mask"].view(np.uint32))
        assert words.tolist() == [0b101, 0b100, 0b111, 0b010]
    for bad in (np.ones((COUNT, NO + 1), dtype=bool), np.ones(NO, dtype=bool), np.ones((COUNT, NO, 1), dtype=bool)):
        with pytest.raises(ValueError, match=rf"active must be \(B, {NO}\), got"):
            m.set_obstacle_mask(bad)
        with pytest.raises(ValueError, match=rf"active must be \(count, {NO}\), got .*n_obst"):
            ep._sweep_features(COUNT, NO, ep.DEFAULT_BOUNDS, active=bad)
    with pytest.raises(ValueError, match=f"the handle holds 1 .. {COUNT} instances"):
        m.set_obstacle_mask(np.ones((COUNT + 1, NO), dtype=bool))
    with pytest.raises(ValueError, match=f"per-seed active has {COUNT + 1} rows for {COUNT} seeds"):
        ep._sweep_features(COUNT, NO, ep.DEFAULT_BOUNDS, active=np.ones((COUNT + 1, NO), dtype=bool))


@pytest.mark.parametrize("name,cols,value", [("bx_lo", 4, -3.0), ("bx_hi", 4, 3.0), ("bu_lo", 2, -2.0), ("bu_hi", 2, 2.0)])
def test_bounds_groups_are_normalised_alike_on_both_sides(ep, monkeypatch, name, cols, value):
    from mpc_gpu.solver import BOUNDS_ROW
    group_cols = dict(bx_lo=4, bx_hi=4, bu_lo=2, bu_hi=2)           # in the order of the C prototype
    m, calls = bare(monkeypatch, lambda fn, a: (fn, a[1], {n: None if p is None else at(p, C.c_double, (a[1], c)) for (n, c), p in zip(group_cols.items(), a[2:])}))
    col0 = {n: c0 for n, c0, _ in BOUNDS_ROW}[name]
    rows = value + np.arange(COUNT * cols).reshape(COUNT, cols) / 100.0
    for a in (rows, rows.tolist(), rows[0], rows[0].tolist()):            # (rows, cols), and one row for all
        calls.clear()
        m.set_instance_bounds(**{name: a})
        (fn, B, given), = calls
        assert fn == "mpc_set_instance_bounds" and B == COUNT and [n for n, g in given.items() if g is not None] == [name]
        batch = given[name]
        sweep = ep._sweep_features(COUNT, NO, ep.DEFAULT_BOUNDS, bounds={name: a})["bounds"]
        assert np.array_equal(batch, sweep[:, col0:col0 + cols]) and np.array_equal(batch, np.broadcast_to(np.asarray(a, dtype=np.float64), (COUNT, cols)))
    for bad in (np.full((COUNT, cols + 1), value), np.full(cols + 1, value), np.full((COUNT, cols, 1), value)):
        with pytest.raises(ValueError, match=rf"{name} must be \(B, {cols}\) or \({cols},\), got"):
            m.set_instance_bounds(**{name: bad})
        with pytest.raises(ValueError, match=rf"{name} must be \(count, {cols}\) or \({cols},\), got"):
            ep._sweep_features(COUNT, NO, ep.DEFAULT_BOUNDS, bounds={name: bad})
    with pytest.raises(ValueError, match=f"per-seed {name} has {COUNT + 1} rows for {COUNT} seeds"):
        ep._sweep_features(COUNT, NO, ep.DEFAULT_BOUNDS, bounds={name: np.full((COUNT + 1, cols), value)})


# ---------------------------------------------------------------------------------------------------------------- 4. the two loops, on fakes
LENGTHS = [2, 5, 1, 3, 3, 1, 4, 2]          # the control steps seed index k runs; every episode ends on its goal
ROWS = {"slots": 2, "groups": 4}            # the res_i columns of run_seed_sweep's rows and of run_multistart_sweep's (lost and switched behind them)


class FakeSweep:
    """a sweep's device side on CPU tensors: `refill` is the refill's rule (multistart_sweep_cases.decide, then park / drain / start on the bookkeeping
    words alone), `step` one control step of every running row; both record their call"""

    def __init__(self, torch, lengths, S, cols):
        i32 = dict(dtype=torch.int32)
        self.torch, self.lengths, self.S, self.cols, self.calls = torch, lengths, S, cols, []
        self.flags, self.steps, self.slot_seed, self.cursor = torch.ones(S, **i32), torch.zeros(S, **i32), torch.full((S,), -1, **i32), torch.zeros(2, **i32)
        self.res_f, self.res_i = torch.full((len(lengths), 6), float("nan"), dtype=torch.float64), torch.full((len(lengths), cols), -1, **i32)

    def refill(self, k):
        import multistart_sweep_cases as sc
        self.calls.append("refill")
        assign, cursor = sc.decide(self.flags.numpy(), self.steps.numpy(), int(self.cursor[0]), len(self.lengths), 10 ** 6)
        for g, s in enumerate(assign.tolist()):
            if s == sc.KEEP:
                continue
            old = int(self.slot_seed[g])
            if old >= 0:          # park: margin 1 + seed, last state (seed, ...), flags, steps and, for groups, lost = seed and switched = 2 seed
                self.res_f[old] = self.torch.tensor([1.0 + old] + [float(old)] * 5, dtype=self.torch.float64)
                self.res_i[old] = self.torch.tensor([int(self.flags[g]), int(self.steps[g]), old, 2 * old][:self.cols], dtype=self.torch.int32)
            if s == sc.DRAIN:
                self.slot_seed[g] = -1; self.flags[g] |= 1
            else:
                self.slot_seed[g] = s; self.flags[g] = 0; self.steps[g] = 0
        self.cursor[:] = self.torch.from_numpy(cursor)

    def step(self, k):
        self.calls.append("step")
        for g in range(self.S):
            if int(self.flags[g]) & 1:
                continue
            ran = int(self.steps[g]) + 1
            if ran == self.lengths[int(self.slot_seed[g])]:
                self.flags[g] |= 1          # (the step that reaches the goal is not counted)
            else:
                self.steps[g] = ran


@pytest.mark.parametrize("noun", list(ROWS))
def test_the_sweep_loop_records_the_models_schedule_and_calls_refill_step_in_turn(ep, no_device, noun):
    import torch
    S = 3
    f = FakeSweep(torch, LENGTHS, S, ROWS[noun])
    k, schedule = ep._sweep_loop(torch, None, S, len(LENGTHS), f.slot_seed, f.cursor, 1, 100, f.refill, f.step)
    want = ep.refill_schedule(LENGTHS, S)
    assert len(set(LENGTHS)) >= 3 and k == want["steps"]
    assert np.array_equal(schedule[:, 0], want["slot"]) and np.array_equal(schedule[:, 1], want["start"])
    assert f.calls == ["refill", "step"] * k + ["refill"]          # one refill per step, and the one that sees no live row
    # the rows the fake has parked, through the drivers' shared collect
    goal = np.array([[3.0, 4.0]])
    table, xl, ri = ep._sweep_table(f.cursor, f.res_i, f.res_f, goal, 100, noun)
    seeds = np.arange(len(LENGTHS))
    assert np.array_equal(table[:, 4] + table[:, 1], LENGTHS) and np.array_equal(table[:, 2], 1.0 + seeds) and np.array_equal(xl, np.repeat(seeds[:, None], 5, axis=1))
    assert ri.shape == (len(LENGTHS), ROWS[noun]) and (noun == "slots" or (np.array_equal(ri[:, 2], seeds) and np.array_equal(ri[:, 3], 2 * seeds)))


def test_the_sweep_loop_stops_at_its_bound_whatever_the_cursor_says(ep, no_device):
    import torch
    calls, bound = [], 5
    slot_seed, cursor = torch.full((2,), -1, dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32)          # cursor[1]: a row that never finishes
    k, schedule = ep._sweep_loop(torch, None, 2, 4, slot_seed, cursor, 1, bound, lambda k: calls.append(("refill", k)), lambda k: calls.append(("step", k)))
    assert k == bound and [c for c in calls if c[0] == "step"] == [("step", j) for j in range(bound)]
    assert [c for c in calls if c[0] == "refill"] == [("refill", j) for j in range(bound + 1)] and (schedule == -1).all()


def test_the_episode_loop_runs_max_iter_steps_and_needs_no_pinned_memory_before_its_first_poll(ep, no_device):
    import torch

    def flags():
        raise AssertionError("no poll is due before control step 25")
    ks = []
    assert ep._episode_loop(torch, None, 7, ks.append, flags) == 7 and ks == list(range(7))
    # the hook that stands in for the poll (run_episodes' compaction): called behind every 25th step, and its False ends the loop
    ks, hooked = [], []
    assert ep._episode_loop(torch, None, 60, ks.append, flags, every_25=lambda k: hooked.append(k) or k < 50) == 50
    assert ks == list(range(50)) and hooked == [25, 50]


@pytest.mark.parametrize("noun", list(ROWS))
def test_the_shared_collect_refuses_a_sweep_that_has_not_drained_and_builds_result_table(ep, no_device, noun):
    import torch
    from mpc_gpu._lib import MpcError
    rng = np.random.default_rng(7)
    count, cols = 5, ROWS[noun]
    ri = np.column_stack([rng.integers(0, 8, count), rng.integers(0, 30, count)] + [rng.integers(0, 9, count)] * (cols - 2)).astype(np.int32)
    rf = rng.uniform(-3.0, 3.0, (count, 6))
    for goal in (rng.uniform(-7.0, 7.0, (1, 2)), rng.uniform(-7.0, 7.0, (count, 2))):          # one goal row for all seeds, and one per seed
        table, xl, raw = ep._sweep_table(torch.tensor([count, 0], dtype=torch.int32), torch.from_numpy(ri), torch.from_numpy(rf), goal, 40, noun)
        assert np.array_equal(table, ep.result_table(ri[:, 0], rf[:, 0], rf[:, 1:6], np.broadcast_to(goal, (count, 2)), ri[:, 1]))
        assert np.array_equal(xl, rf[:, 1:6]) and xl.flags["C_CONTIGUOUS"] and np.array_equal(raw, ri) and table.shape == (count, 6)
    unparked = ri.copy(); unparked[3] = -1
    with pytest.raises(MpcError, match=rf"did not drain within 40 control steps \(0 {noun} live, 1 rows not parked\)"):
        ep._sweep_table(torch.tensor([count, 0], dtype=torch.int32), torch.from_numpy(unparked), torch.from_numpy(rf), goal, 40, noun)
    with pytest.raises(MpcError, match=rf"did not drain within 40 control steps \(2 {noun} live, 0 rows not parked\)"):
        ep._sweep_table(torch.tensor([count, 2], dtype=torch.int32), torch.from_numpy(ri), torch.from_numpy(rf), goal, 40, noun)
