"""Per-seed feature tables, the device status log and the ring of seeded episodes in a seed sweep, on the GPU.

The yardstick is test_gpu_sweep.py's: run_episodes on ONE batch that holds every seed, compaction off, given the same per-instance arrays
(sweep_feature_cases.batch_feature_reference).  The feature kernels run one instance per wavefront, so a sweep's rows equal that batch's rows BIT FOR BIT
(np.array_equal on table and x_last), whatever slot and control step a seed starts at, and whether its generator was seeded in place or copied from the ring."""
import numpy as np
import pytest

import sweep_cases as sc
import sweep_feature_cases as fc
from feature_loop import Banded
from test_gpu_sweep import STEP_FLAGS, assert_rows_equal, sweep

pytestmark = pytest.mark.gpu

SHAPES = {"24-through-4": (0, 24, 4), "offset-10-through-3": (37, 10, 3)}


@pytest.fixture
def mg(built):
    import mpc_gpu
    mpc_gpu.BatchedMpc.default_lanes_per_stage = 0
    return mpc_gpu


# ---------------------------------------------------------------------------------------------------------------- 1. each feature alone, then all together
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("name", sorted(fc.FEATURES))
def test_per_seed_features_are_the_batch_harness_bit_for_bit(mg, name, shape):
    first, count, slots = SHAPES[shape]
    ref = fc.batch_feature_reference(mg, "RANDOM", first, count, name)
    plain = sc.batch_reference(mg, "RANDOM", first, count)
    assert not np.array_equal(ref["table"], plain["table"]), "the yardstick itself: the per-instance arrays change the batch's rows"
    r = sweep(mg, "RANDOM", (first, count), slots, **fc.feature_kwargs(name, count))
    assert_rows_equal(r, ref)
    assert r["solves"] == ref["solves"]


def test_weights_yardstick_is_a_handle_with_instance_params(mg):
    """W / We have no run_episodes argument: the yardstick is run_episodes(solver=m) on a handle with set_instance_params(W=, We=), and a sweep on a
    caller's handle leaves that handle as it came"""
    ref = fc.batch_feature_reference(mg, "RANDOM", 0, 24, "weights")
    with mg.BatchedMpc(max_batch=6, **sc.PROBLEM) as m:
        r = mg.run_seed_sweep(sc.START, sc.GOAL, "RANDOM", (0, 24), 4, solver=m, **fc.feature_kwargs("weights", 24))
        assert_rows_equal(r, ref)
        again = mg.run_seed_sweep(sc.START, sc.GOAL, "RANDOM", (0, 24), 4, solver=m)          # nothing is left behind: the plain sweep
        assert_rows_equal(again, sc.batch_reference(mg, "RANDOM", 0, 24))


# ---------------------------------------------------------------------------------------------------------------- 2. the status log
LOW_QP = dict(sc.PROBLEM, qp_iter_max=8)


def test_status_log_is_run_episodes_status_log(mg):
    x0, g = np.tile(sc.START, (24, 1)), np.tile(sc.GOAL, (24, 1))
    ref = mg.run_episodes(x0, g, "RANDOM", first_seed=0, compact_from=None, status_log=True, max_iter=80, **LOW_QP)
    print("yardstick status2", int(ref["status2"].sum()), "status4", int(ref["status4"].sum()), "episodes with a bad step", int((ref["first_bad"] >= 0).sum()))
    assert ref["status2"].sum() > 0 and (ref["first_bad"] >= 0).any(), "the yardstick itself shows a status 2"
    assert len(set(ref["status2"].tolist())) > 1, "... and not the same count for every seed: rows parked under a wrong seed would show"
    r = sweep(mg, "RANDOM", (0, 24), 4, problem=LOW_QP, max_iter=80, status_log=True)
    assert_rows_equal(r, ref)
    for n in ("status2", "status4", "first_bad"):
        assert np.array_equal(r[n], ref[n]), n
    both = sweep(mg, "RANDOM", (0, 24), 4, problem=LOW_QP, max_iter=80, status_log=True, ring=2, ring_every=10, **fc.feature_kwargs("radii", 24))
    rad = mg.run_episodes(x0, g, "RANDOM", first_seed=0, compact_from=None, status_log=True, max_iter=80, **LOW_QP, **fc.feature_kwargs("radii", 24))
    assert_rows_equal(both, rad)
    for n in ("status2", "status4", "first_bad"):
        assert np.array_equal(both[n], rad[n]), n


# ---------------------------------------------------------------------------------------------------------------- 3. the ring
@pytest.mark.parametrize("capacity", [2, 4, 7])
def test_ring_rows_schedule_and_source(mg, capacity):
    """poll_every = 1 records the schedule: rows are the ring-off sweep's and the batch's, the schedule is the slot-order model's, and which seeds came
    from the ring is the ring model's -- at capacity 2 both the copy and the in-place seeding have run"""
    ref = sc.batch_reference(mg, "RANDOM", 0, 24)
    off = sweep(mg, "RANDOM", range(24), 4, poll_every=1)
    r = sweep(mg, "RANDOM", range(24), 4, poll_every=1, ring=capacity, ring_every=10)
    assert_rows_equal(r, ref)
    assert np.array_equal(r["table"], off["table"]) and np.array_equal(r["x_last"], off["x_last"]) and "seed_src" not in off
    want = mg.refill_schedule((ref["table"][:, 4] + ref["table"][:, 1]).astype(int), 4)
    assert np.array_equal(r["schedule"][:, 0], want["slot"]) and np.array_equal(r["schedule"][:, 1], want["start"]) and r["steps_run"] == want["steps"]
    model = mg.ring_model(r["schedule"][:, 1], capacity, 10)
    assert np.array_equal(r["seed_src"], model), (r["seed_src"], model)
    if capacity == 2:
        assert set(r["seed_src"].tolist()) == {0, 1}
        assert r["seed_src"][:4].tolist() == [1, 1, 0, 0]


def test_ring_with_every_table(mg):
    ref = fc.batch_feature_reference(mg, "RANDOM", 0, 24, "all")
    r = sweep(mg, "RANDOM", range(24), 4, poll_every=1, ring=2, ring_every=10, **fc.feature_kwargs("all", 24))
    assert_rows_equal(r, ref)
    assert np.array_equal(r["seed_src"], mg.ring_model(r["schedule"][:, 1], 2, 10)) and set(r["seed_src"].tolist()) == {0, 1}
    timed = sweep(mg, "RANDOM", range(24), 4, ring=4, **fc.feature_kwargs("all", 24))           # the timed form: polled, filled every poll
    assert_rows_equal(timed, ref)
    assert "seed_src" not in timed


def test_ring_edge(mg):
    ref = sc.batch_reference(mg, "EDGE", 37, 10)
    r = sweep(mg, "EDGE", (37, 10), 3, poll_every=1, ring=2, ring_every=7)
    assert_rows_equal(r, ref)
    assert np.array_equal(r["seed_src"], mg.ring_model(r["schedule"][:, 1], 2, 7))


def test_ring_with_more_than_ten_obstacles(mg):
    """15 obstacles: the scenario draw regenerates the generator, in the ring fill as in the refill"""
    ref = sc.batch_reference(mg, "RANDOM", 0, 8, problem=sc.WIDE_PROBLEM, max_iter=60)
    r = sweep(mg, "RANDOM", range(8), 4, problem=sc.WIDE_PROBLEM, max_iter=60, poll_every=1, ring=3, ring_every=5)
    assert_rows_equal(r, ref)
    assert np.array_equal(r["seed_src"], mg.ring_model(r["schedule"][:, 1], 3, 5)) and r["seed_src"][:3].tolist() == [1, 1, 1]


def test_ring_refuses_a_refill_for_another_sweep(mg):
    """filled with one seed_first, refilled with another: MPC_ERR_ARG, and nothing written"""
    import torch
    from mpc_gpu import _lib
    with mg.BatchedMpc(max_batch=4, **sc.PROBLEM) as m:
        arr = sc.SlotArrays(sc.Plain(torch, torch.device("cuda", 0)), m, 4, 12, _lib.lib().mpc_noise_state_words())
        ft = fc.FeatureArrays(sc.Plain(torch, torch.device("cuda", 0)), m, 12, capacity=3, total=24)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            m.episode_ring_fill_dev("RANDOM", 0, 12, arr.cursor, stream=stream.cuda_stream)
            stream.synchronize()
            assert ft.ring_tag.cpu().tolist() == [0, 1, 2]
            before, fbefore = arr.snapshot(), ft.snapshot()
            for first, count, scenario in ((5, 12, "RANDOM"), (0, 11, "RANDOM"), (0, 12, "EDGE")):
                with pytest.raises(mg.MpcError, match="ring") as e:
                    arr.refill(m, scenario, first, 400, _lib.REFILL_ALIAS_BUG | _lib.REFILL_DRAW_NOISE, stream.cuda_stream, count=count)
                assert f"error {_lib.MPC_ERR_ARG}" in str(e.value)
            stream.synchronize()
            after, fafter = arr.snapshot(), ft.snapshot()
            for n in sc.ALL_ARRAYS:
                assert np.array_equal(before[n], after[n], equal_nan=True), n
            for n in ft.names:
                assert np.array_equal(fbefore[n], fafter[n]), n
            arr.refill(m, "RANDOM", 0, 400, _lib.REFILL_ALIAS_BUG | _lib.REFILL_DRAW_NOISE, stream.cuda_stream)       # the sweep it was filled for goes through
            stream.synchronize()
        assert arr.slot_seed.cpu().tolist() == [0, 1, 2, 3] and ft.seed_src.cpu().tolist()[:4] == [1, 1, 1, 0]
        with pytest.raises(mg.MpcError, match="slot_W"):             # a source without its destination names the field
            m.set_refill_tables_dev(W=ft.W)
        m.set_refill_tables_dev(); m.episode_ring_dev(0)


# ---------------------------------------------------------------------------------------------------------------- 4. guard bands, and a refill with nothing finished
def drive_features(torch, m, arr, ft, first, count, ring_every, bound):
    """fill (every ring_every steps) -> refill -> fused step -> status log, until no slot runs"""
    from mpc_gpu import _lib
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    k = 0
    with torch.cuda.stream(stream):
        while True:
            if k % ring_every == 0:
                m.episode_ring_fill_dev("RANDOM", first, count, arr.cursor, stream=stream.cuda_stream)
            arr.refill(m, "RANDOM", first, 400, _lib.REFILL_ALIAS_BUG | _lib.REFILL_DRAW_NOISE, stream.cuda_stream)
            stream.synchronize()
            if int(arr.cursor[1].item()) == 0:
                break
            assert k < bound
            step_flags = STEP_FLAGS | _lib.STEP_MARGIN_ALL
            arr.step(m, step_flags, stream.cuda_stream)
            m.episode_status_log_dev(arr.slots, arr.status, arr.flags, arr.steps, ft.log, stream=stream.cuda_stream)
            k += 1
        stream.synchronize()
    return k


def test_guard_bands_and_rows_beyond_the_slots(mg):
    """every array the new launches write sits between sentinel words -- per-slot tables, log, res_log, the ring arrays, seed_src: 12 seeds through 4 slots
    of a handle of 6, every feature on, and the bands are as they were; rows 4 and 5 of the per-slot arrays are never written"""
    import torch
    from mpc_gpu import _lib
    ref = fc.batch_feature_reference(mg, "RANDOM", 0, 24, "all")
    with mg.BatchedMpc(max_batch=6, **sc.PROBLEM) as m:
        bands = Banded(torch, torch.device("cuda", 0))
        arr = sc.SlotArrays(bands, m, 4, 12, _lib.lib().mpc_noise_state_words())
        ft = fc.FeatureArrays(bands, m, 12, capacity=3, total=24)
        torch.cuda.synchronize()
        preset = ft.snapshot(slice(4, 6))
        k = drive_features(torch, m, arr, ft, 0, 12, 10, 3 * 400)
        assert bands.intact()
        last = ft.snapshot(slice(4, 6))
        table, xl = arr.table()
        res_log, seed_src, tags = ft.res_log.cpu().numpy(), ft.seed_src.cpu().numpy(), ft.ring_tag.cpu().numpy()
        m.set_refill_tables_dev(); m.episode_ring_dev(0)
    for n in fc.TABLE_ARRAYS:
        assert np.array_equal(preset[n], last[n]), n
    assert np.array_equal(table, ref["table"][:12]) and np.array_equal(xl, ref["x_last"][:12])
    lengths = (ref["table"][:12, 4] + ref["table"][:12, 1]).astype(int)
    want = mg.refill_schedule(lengths, 4)
    assert k == want["steps"]
    assert np.array_equal(seed_src, mg.ring_model(want["start"], 3, 10))
    assert (res_log[:, :2] >= 0).all() and (res_log[:, 2] >= -1).all() and (res_log[:, 2] < lengths).all()
    assert all(0 <= t < 12 and t % 3 == e for e, t in enumerate(tags.tolist()))        # entry e only ever holds an index k with k % capacity == e


def test_a_refill_with_nothing_finished_changes_no_table(mg):
    import torch
    from mpc_gpu import _lib
    with mg.BatchedMpc(max_batch=6, **sc.PROBLEM) as m:
        plain = sc.Plain(torch, torch.device("cuda", 0))
        arr = sc.SlotArrays(plain, m, 6, 20, _lib.lib().mpc_noise_state_words())
        ft = fc.FeatureArrays(plain, m, 20, capacity=4, total=24)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            m.episode_ring_fill_dev("EDGE", 3, 20, arr.cursor, stream=stream.cuda_stream)
            for _ in range(5):
                arr.refill(m, "EDGE", 3, 400, _lib.REFILL_ALIAS_BUG | _lib.REFILL_DRAW_NOISE, stream.cuda_stream)
                arr.step(m, STEP_FLAGS, stream.cuda_stream)
                m.episode_status_log_dev(6, arr.status, arr.flags, arr.steps, ft.log, stream=stream.cuda_stream)
            stream.synchronize()
            before, fbefore = arr.snapshot(), ft.snapshot()
            assert ((before["flags"] & 1) == 0).all() and (before["steps"] == 5).all() and before["slot_seed"].tolist() == list(range(6))
            assert fbefore["log"][:, 3].tolist() == [5] * 6 and fbefore["ring_tag"].tolist() == [0, 1, 2, 3]
            assert not np.array_equal(fbefore["slot_W"], np.tile(fc.HANDLE["W"], (6, 1)))          # (the tables were copied when the seeds started)
            arr.refill(m, "EDGE", 3, 400, _lib.REFILL_ALIAS_BUG, stream.cuda_stream)
            stream.synchronize()
            after, fafter = arr.snapshot(), ft.snapshot()
        m.set_refill_tables_dev(); m.episode_ring_dev(0)
    for n in sc.ALL_ARRAYS:
        assert np.array_equal(before[n], after[n], equal_nan=True), n
    for n in ft.names:
        assert np.array_equal(fbefore[n], fafter[n]), n
    assert np.array_equal(ft.seed_src.cpu().numpy()[:6], [1, 1, 1, 1, 0, 0])
