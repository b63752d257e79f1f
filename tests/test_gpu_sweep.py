"""Seed sweeps with on-device episode refill (mpc_episode_refill_dev, run_seed_sweep) on the GPU.

The yardstick is the path that exists without the sweep: run_episodes on ONE batch that holds every seed (sweep_cases.batch_reference, compaction off).
With one instance per wavefront an episode's arithmetic is its own, so a sweep through a few slots must return that batch's rows BIT FOR BIT, whatever
slot and control step a seed starts at; the recorded tables of the reference pin the absolute values.  Sizes are the smallest at which a refill can go
wrong: more seeds than slots, counts that are no multiple of the slots, an offset first seed, slots that outnumber the seeds."""
import ctypes as C
import os

import numpy as np
import pytest

import sweep_cases as sc
from feature_loop import Banded

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["stage-split", "one-lane-per-stage"])
def mapping(built, request):
    """function-scoped: the class attribute is restored behind every test (as tests/test_gpu_replay.py does)"""
    import mpc_gpu
    mpc_gpu.BatchedMpc.default_lanes_per_stage = 0 if request.param == "stage-split" else 1
    yield mpc_gpu
    mpc_gpu.BatchedMpc.default_lanes_per_stage = 0


@pytest.fixture
def mg(built):
    import mpc_gpu
    mpc_gpu.BatchedMpc.default_lanes_per_stage = 0
    return mpc_gpu


def sweep(mpc_gpu, scenario, seeds, slots, start=sc.START, goal=sc.GOAL, problem=sc.PROBLEM, **kw):
    return mpc_gpu.run_seed_sweep(start, goal, scenario, seeds, slots, **problem, **kw)


def assert_rows_equal(r, ref, rows=slice(None)):
    assert np.array_equal(r["table"], ref["table"][rows]), np.nonzero((r["table"] != ref["table"][rows]).any(axis=1))[0]
    assert np.array_equal(r["x_last"], ref["x_last"][rows])


# ---------------------------------------------------------------------------------------------------------------- 4. the reference's recorded rows
@pytest.mark.parametrize("scen", ["RANDOM", "EDGE"])
def test_recorded_rows(mg, scen):
    """seeds 0 .. 99 through 16 slots: on the seeds the reference's own tables prove converged (STABLE of test_gpu_replay.py) the control-step count and the
    three flags are the recorded ones exactly, min_margin within 1e-4 and dist_to_goal within 1e-3 -- the bounds tests/test_gpu_replay.py holds those tables to"""
    from test_gpu_replay import STABLE, TABLES
    rows = np.array(TABLES[sc.RECORDED[scen]]["rows"])
    assert TABLES[sc.RECORDED[scen]]["spec"]["scenario"] == scen and TABLES[sc.RECORDED[scen]]["spec"]["QP_ITER"] == 100
    r = sweep(mg, scen, range(100), 16)
    tb, st = r["table"], STABLE[scen]
    print(scen, "steps_run", r["steps_run"], "max |min_margin - recorded|", np.abs(tb[st, 2] - rows[st, 2]).max(), "max |dist - recorded|", np.abs(tb[st, 3] - rows[st, 3]).max())
    assert np.array_equal(tb[st, 4], rows[st, 4]), (tb[st, 4], rows[st, 4])
    assert np.array_equal(tb[st][:, [0, 1, 5]], rows[st][:, [0, 1, 5]])
    assert np.abs(tb[st, 2] - rows[st, 2]).max() <= 1e-4
    assert np.abs(tb[st, 3] - rows[st, 3]).max() <= 1e-3
    assert r["solves"] == int(tb[:, 4].sum() + tb[:, 1].sum()) and r["schedule"] is None


# ---------------------------------------------------------------------------------------------------------------- 5. bit for bit the batch harness
@pytest.mark.parametrize("scen", ["RANDOM", "EDGE"])
def test_sweep_is_the_batch_harness_bit_for_bit(mapping, scen):
    ref = sc.batch_reference(mapping, scen, 0, 40)
    r = sweep(mapping, scen, range(40), 8)
    assert_rows_equal(r, ref)
    assert r["solves"] == ref["solves"]
    lengths = (ref["table"][:, 4] + ref["table"][:, 1]).astype(int)
    want = mapping.refill_schedule(lengths, 8)["steps"]
    assert r["steps_run"] == min((-(-want // 25) + 1) * 25, 5 * 400 + 25), (r["steps_run"], want)       # polled every 25 steps, looked at one poll later


@pytest.mark.parametrize("scen", ["RANDOM", "EDGE"])
def test_offset_first_seed_and_a_count_that_is_no_multiple_of_the_slots(mapping, scen):
    ref = sc.batch_reference(mapping, scen, 37, 10)
    assert_rows_equal(sweep(mapping, scen, (37, 10), 3), ref)
    assert np.array_equal(ref["table"][:3], sc.batch_reference(mapping, scen, 0, 40)["table"][37:40])      # (the yardstick itself: seed 37 + s is seed 37 + s)


# ---------------------------------------------------------------------------------------------------------------- 6. the schedule
def test_schedule_is_the_slot_order_model_and_repeats(mg):
    ref = sc.batch_reference(mg, "RANDOM", 0, 40)
    lengths = (ref["table"][:24, 4] + ref["table"][:24, 1]).astype(int)
    want = mg.refill_schedule(lengths, 4)
    a = sweep(mg, "RANDOM", range(24), 4, poll_every=1)
    b = sweep(mg, "RANDOM", range(24), 4, poll_every=1)
    assert_rows_equal(a, ref, slice(0, 24))
    assert np.array_equal(a["schedule"][:, 0], want["slot"]) and np.array_equal(a["schedule"][:, 1], want["start"])
    assert a["steps_run"] == want["steps"] == b["steps_run"]
    assert np.array_equal(a["schedule"], b["schedule"]) and np.array_equal(a["table"], b["table"])


# ---------------------------------------------------------------------------------------------------------------- 7. the budget
def test_budget_spent_counts_as_finished(mg):
    ref = sc.batch_reference(mg, "RANDOM", 0, 10, max_iter=12)
    r = sweep(mg, "RANDOM", range(10), 4, max_iter=12, poll_every=1)
    assert (r["table"][:, 4] == 12).all() and (r["table"][:, 1] == 0).all()
    assert r["steps_run"] == 36
    assert_rows_equal(r, ref)
    assert r["schedule"].tolist() == [[s, 0] for s in range(4)] + [[s, 12] for s in range(4)] + [[0, 24], [1, 24]]


# ---------------------------------------------------------------------------------------------------------------- 8, 9, 10, 13: the entry point itself
STEP_FLAGS = 1 | 2 | 4 | 32 | 8 | 16            # shift, plant, obstacles, metrics, reset on fail with the aliasing defect: what run_episodes sets by default


def drive(torch, m, arr, scenario, first, max_steps, refill_flags, bound, after_first=None):
    """refill -> fused step until no slot runs; returns the fused steps launched"""
    torch.cuda.synchronize()            # (the arrays were preset on torch's default stream)
    stream = torch.cuda.Stream()
    k = 0
    with torch.cuda.stream(stream):
        while True:
            arr.refill(m, scenario, first, max_steps, refill_flags, stream.cuda_stream)
            stream.synchronize()
            if k == 0 and after_first is not None:
                after_first()
            if int(arr.cursor[1].item()) == 0:
                break
            assert k < bound
            arr.step(m, STEP_FLAGS, stream.cuda_stream)
            k += 1
        stream.synchronize()
    return k


def test_more_slots_than_seeds(mg):
    """5 seeds in 8 slots: the rows are the batch harness's, and the three surplus slots are never written behind the first call"""
    import torch
    ref = sc.batch_reference(mg, "RANDOM", 0, 5)
    assert_rows_equal(sweep(mg, "RANDOM", range(5), 8), ref)        # (run_seed_sweep allocates min(slots, count) slots)
    from mpc_gpu import _lib
    with mg.BatchedMpc(max_batch=8, **sc.PROBLEM) as m:
        arr = sc.SlotArrays(sc.Plain(torch, torch.device("cuda", 0)), m, 8, 5, _lib.lib().mpc_noise_state_words())
        preset = arr.snapshot(sc.SLOT_ARRAYS, slice(5, 8))
        first = {}
        k = drive(torch, m, arr, "RANDOM", 0, 400, _lib.REFILL_ALIAS_BUG | _lib.REFILL_DRAW_NOISE, 400, after_first=lambda: first.update(arr.snapshot(sc.SLOT_ARRAYS, slice(5, 8))))
        last = arr.snapshot(sc.SLOT_ARRAYS, slice(5, 8))
        table, xl = arr.table()
    for n in sc.SLOT_ARRAYS:
        assert np.array_equal(preset[n], first[n], equal_nan=True) and np.array_equal(first[n], last[n], equal_nan=True), n
    assert np.array_equal(table, ref["table"]) and np.array_equal(xl, ref["x_last"])
    assert k == int((ref["table"][:, 4] + ref["table"][:, 1]).max())
    assert arr.slot_seed.cpu().tolist() == [-1] * 8 and arr.cursor.cpu().tolist() == [5, 0] and (arr.flags.cpu().numpy() & 1).all()


def test_a_call_with_nothing_finished_changes_nothing(mg):
    import torch
    from mpc_gpu import _lib
    with mg.BatchedMpc(max_batch=6, **sc.PROBLEM) as m:
        arr = sc.SlotArrays(sc.Plain(torch, torch.device("cuda", 0)), m, 6, 20, _lib.lib().mpc_noise_state_words())
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            for _ in range(5):
                arr.refill(m, "EDGE", 3, 400, _lib.REFILL_ALIAS_BUG | _lib.REFILL_DRAW_NOISE, stream.cuda_stream)
                arr.step(m, STEP_FLAGS, stream.cuda_stream)
            stream.synchronize()
            before = arr.snapshot()
            assert ((before["flags"] & 1) == 0).all() and (before["steps"] == 5).all() and before["slot_seed"].tolist() == list(range(6)) and before["cursor"].tolist() == [6, 6]
            arr.refill(m, "EDGE", 3, 400, _lib.REFILL_ALIAS_BUG, stream.cuda_stream)
            stream.synchronize()
            after = arr.snapshot()
    for n in sc.ALL_ARRAYS:
        assert np.array_equal(before[n], after[n], equal_nan=True), n


def test_guard_bands_stay_intact(mg):
    """every array the refill writes sits between sentinel words: 12 seeds through 4 slots, and the bands are as they were"""
    import torch
    from mpc_gpu import _lib
    ref = sc.batch_reference(mg, "RANDOM", 0, 40)
    with mg.BatchedMpc(max_batch=4, **sc.PROBLEM) as m:
        bands = Banded(torch, torch.device("cuda", 0))
        arr = sc.SlotArrays(bands, m, 4, 12, _lib.lib().mpc_noise_state_words())
        k = drive(torch, m, arr, "RANDOM", 0, 400, _lib.REFILL_ALIAS_BUG | _lib.REFILL_DRAW_NOISE, 3 * 400)
        assert bands.intact()
        table, xl = arr.table()
    assert np.array_equal(table, ref["table"][:12]) and np.array_equal(xl, ref["x_last"][:12])
    assert k == mg.refill_schedule((ref["table"][:12, 4] + ref["table"][:12, 1]).astype(int), 4)["steps"]


def test_argument_refusals_through_the_c_abi(mg):
    """MPC_ERR_ARG with a message, and nothing launched: the preset arrays are what they were"""
    import torch
    from mpc_gpu import _lib
    from mpc_gpu.solver import _ptr
    L = _lib.lib()
    with mg.BatchedMpc(max_batch=4, **sc.PROBLEM) as m:
        arr = sc.SlotArrays(sc.Plain(torch, torch.device("cuda", 0)), m, 4, 12, L.mpc_noise_state_words())
        torch.cuda.synchronize()
        before = arr.snapshot()
        box = m._scenario_box()
        stream = torch.cuda.Stream()

        def call(slots=4, scenario=0, seed_count=12, max_steps=400, flags=_lib.REFILL_DRAW_NOISE, per_seed=0, **null):
            p = {n: _ptr(getattr(arr, n)) for n in sc.ALL_ARRAYS}
            p.update({n: None for n in null})
            return L.mpc_episode_refill_dev(m._h, slots, scenario, 0, seed_count, max_steps, flags, _ptr(box), _ptr(arr.start_rows), _ptr(arr.goal_rows), per_seed,
                                            *[p[n] for n in sc.ALL_ARRAYS], C.c_void_p(stream.cuda_stream))
        for kw, word in ((dict(slots=5), b"slots"), (dict(slots=0), b"slots"), (dict(max_steps=0), b"max_steps"), (dict(scenario=3), b"scenario"),
                         (dict(res_f=True), b"result"), (dict(res_i=True), b"result"), (dict(seed_count=-1), b"seed_count"), (dict(flags=8), b"flag"),
                         (dict(noise=True), b"noise"), (dict(slot_seed=True), b"slot_seed"), (dict(per_seed=2), b"per_seed")):
            assert call(**kw) == _lib.MPC_ERR_ARG, kw
            assert word in L.mpc_last_error(), (kw, L.mpc_last_error())
        torch.cuda.synchronize()
        after = arr.snapshot()
        for n in sc.ALL_ARRAYS:
            assert np.array_equal(before[n], after[n], equal_nan=True), n
        assert call(flags=0, noise=True) == 0          # (without the noise flag the noise array may be null) ... and a good call fills the slots
        torch.cuda.synchronize()
        assert arr.slot_seed.cpu().tolist() == [0, 1, 2, 3] and arr.cursor.cpu().tolist() == [4, 4]


# ---------------------------------------------------------------------------------------------------------------- 11. options
OPTIONS = {"interp-guess": dict(interpolate_init=True, bug_compat_alias=False), "no-reset": dict(init_guess_when_error=False),
           "still-obstacles": dict(random_move=False), "sqp": dict(sqp=(3, 1e-6))}


@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_options_against_the_batch_harness(mg, name):
    ref = sc.batch_reference(mg, "RANDOM", 0, 12, max_iter=80, **OPTIONS[name])
    r = sweep(mg, "RANDOM", range(12), 4, max_iter=80, **OPTIONS[name])
    assert_rows_equal(r, ref)


def test_per_seed_start_and_goal(mg):
    start, goal = sc.per_seed_rows(12)
    assert len({tuple(r) for r in start}) == 12 and len({tuple(r) for r in goal}) == 12
    ref = sc.batch_reference(mg, "RANDOM", 0, 12, start=start, goal=goal, max_iter=80)
    r = sweep(mg, "RANDOM", range(12), 4, start=start, goal=goal, max_iter=80)
    assert_rows_equal(r, ref)
    one = sweep(mg, "RANDOM", range(12), 4, start=start, max_iter=80)          # per-seed start with ONE goal row
    assert np.array_equal(one["table"], sc.batch_reference(mg, "RANDOM", 0, 12, start=start, max_iter=80)["table"])


# ---------------------------------------------------------------------------------------------------------------- 12. more than ten obstacles
@pytest.mark.parametrize("scen", ["RANDOM", "EDGE"])
def test_more_than_ten_obstacles(mg, scen):
    """N 10, 15 obstacles, Tf 1: the multi-wavefront solve kernel, and scenario draws that reach past the generator's first regeneration words"""
    with mg.BatchedMpc(max_batch=4, **sc.WIDE_PROBLEM) as probe:
        assert "rti_wide_kernel" in probe.kernel_name(4)
    ref = sc.batch_reference(mg, scen, 0, 8, problem=sc.WIDE_PROBLEM, max_iter=60)
    assert_rows_equal(sweep(mg, scen, range(8), 4, problem=sc.WIDE_PROBLEM, max_iter=60), ref)


def test_run_grid_cell_as_a_sweep(mg, tmp_path):
    """run_grid(slots=): a cell with more seeds than slots runs as a sweep and writes the rows of the one-batch cell"""
    a = mg.run_grid(TF=(2,), N_OBST=(5,), QP_ITER=(100,), scenarios=("EDGE",), seeds=10, max_iter=60, out_dir=str(tmp_path / "a"))
    b = mg.run_grid(TF=(2,), N_OBST=(5,), QP_ITER=(100,), scenarios=("EDGE",), seeds=10, max_iter=60, out_dir=str(tmp_path / "b"), slots=4)
    assert np.array_equal(a[0]["table"], b[0]["table"]) and a[0]["spec"] == b[0]["spec"]
    assert os.path.exists(tmp_path / "b" / "grid_EDGE_TF2_N5_QP100_experiment_data.csv")
