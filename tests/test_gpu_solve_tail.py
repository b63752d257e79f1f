"""What the four solve tails must agree on.  The work behind the interior-point loop exists four times -- rti_solve_kernel, the FX and the older order of
rti_split_kernel, rti_wide_kernel -- around a few shared pieces (csrc/rti_kernel.hpp "the solve tail"); an edit of the shared pieces,
or of one copy and not the others, is checked here on every one.
Per tail variant, at the smallest shape that runs it (N = 5, B = 5, three control steps; kernel_name asserts that the intended kernel runs):
  * one fused control step == solve, plant step, obstacle step and shift through their own entry points, bit for bit (helpers.fused_step_is_the_separate_calls),
    with and without velocity noise;
  * the same with a NaN obstacle state in instance 1 and STEP_RESET_ON_FAIL (the separate side resets with reset_guess): instance 1 fails (status 4), its
    neighbours' outputs are those of the clean run, the iterate it is left with is the host reset (shifted, as the step stores it);
  * the result stores: the accumulators of set_accumulators hold the sum of the iteration counts and the number of failed solves."""
import numpy as np
import pytest

from helpers import ARENA, fused_step_is_the_separate_calls, wall_batch

pytestmark = pytest.mark.gpu

B, N, STEPS = 5, 5, 3

# name: (obstacles, lanes per stage (0: default dispatch), lanes per instance, wavefronts per SIMD, what the kernel name starts with)
TAILS = {
    "one-lane-16": (3, 1, 0, 0, "rti_solve_kernel<3, 16,"),         # several instances per wavefront
    "one-lane-64": (3, 1, 64, 0, "rti_solve_kernel<3, 64,"),        # one instance per wavefront
    "split-fx": (3, 3, 0, 1, "rti_split_kernel<3, 3, false"),       # the reordered epilogue
    "split-w2": (3, 2, 0, 2, "rti_split_kernel<3, 2, true"),        # the older order, 256 registers
    "split-lps2-10": (10, 2, 0, 1, "rti_split_kernel<10, 2, false"),    # the older order, ten row pairs on two lanes per stage
    "wide": (11, 0, 0, 0, "rti_wide_kernel<20, 2,"),
}


@pytest.fixture
def env(built):
    import mpc_gpu
    return mpc_gpu


def configure_for(tail):
    no, lps, lpi, waves, prefix = TAILS[tail]

    def configure(s):
        if lps:
            s.set_lanes_per_stage(lps)
        if lpi:
            s.set_lanes_per_instance(lpi)
        if waves:
            s.set_waves_per_simd(waves)
        assert s.kernel_name(B).startswith(prefix), (tail, s.kernel_name(B))
    return no, configure


def batch_for(no):
    x0, goal, obst = wall_batch(B, no, seed=5200 + N)
    obst[3, 0] = [ARENA - 0.1, -ARENA + 0.1, 1.8, -1.8]      # ground-truth reflections as well: the step moves x with vx
    return x0, goal, obst


def step_flags():
    from mpc_gpu import _lib
    return _lib.STEP_SHIFT | _lib.STEP_PLANT | _lib.STEP_OBSTACLES, _lib.STEP_RESET_ON_FAIL


@pytest.mark.parametrize("tail", list(TAILS))
def test_fused_step_is_the_separate_calls_on_every_tail(env, tail):
    mpc_gpu = env
    no, configure = configure_for(tail)
    x0, goal, obst = batch_for(no)
    flags, reset = step_flags()
    noise = np.random.default_rng(77).standard_normal((STEPS, B, no, 2))
    clean = fused_step_is_the_separate_calls(mpc_gpu, N, no, x0, goal, obst, None, configure, flags, steps=STEPS)
    fused_step_is_the_separate_calls(mpc_gpu, N, no, x0, goal, obst, noise, configure, flags, steps=STEPS)
    # a NaN in instance 1's obstacle states: it fails alone, and is reset
    bad = obst.copy(); bad[1, 2, 1] = np.nan
    nan = fused_step_is_the_separate_calls(mpc_gpu, N, no, x0, goal, bad, None, configure, flags | reset, steps=STEPS)
    with mpc_gpu.BatchedMpc(N, no, 0.1 * N, max_batch=B) as s:      # the host reset at the state instance 1 starts from, stored shifted (it is the same in every stage)
        s.reset_guess(x0)
        s.shift(B)
        Xr, Ur = s.get_traj(B)
    others = [b for b in range(B) if b != 1]
    for k in range(STEPS):
        assert nan[k]["status"][1] == 4, k
        assert (clean[k]["status"][others] != 4).all(), k
        for key in ("X", "U", "x", "obst", "u0", "cost", "status", "iters"):
            assert np.array_equal(nan[k][key][others], clean[k][key][others]), (k, key)
        # the failed instance applies u = U[0] = 0 at v = omega = 0: its plant does not move, and every reset is the first one
        assert np.array_equal(nan[k]["x"][1], x0[1]), k
        assert np.array_equal(nan[k]["X"][1], Xr[1]) and np.array_equal(nan[k]["U"][1], Ur[1]), k


@pytest.mark.parametrize("tail", list(TAILS))
def test_accumulators_hold_the_sums_on_every_tail(env, tail):
    import torch
    mpc_gpu = env
    no, configure = configure_for(tail)
    x0, goal, obst = batch_for(no)
    obst[1, 2, 1] = np.nan          # one failed solve per step
    flags, reset = step_flags()
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    with mpc_gpu.BatchedMpc(N, no, 0.1 * N, max_batch=B) as s, torch.cuda.stream(torch.cuda.Stream(device=dev)):
        configure(s)
        s.reset_guess(x0)
        st = torch.cuda.current_stream().cuda_stream
        iters_acc = torch.zeros(B, dtype=torch.int32, device=dev); status_acc = torch.zeros(B, dtype=torch.int32, device=dev)
        s.set_accumulators(iters_acc, status_acc)
        dx, dobst, dgoal = t(x0), t(obst), t(goal)
        status = torch.zeros(B, dtype=torch.int32, device=dev); iters = torch.zeros(B, dtype=torch.int32, device=dev)
        dX, dU, _ = s.iterate_ptrs()
        it_sum, failed, capped = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int64)
        for k in range(STEPS):
            s.closed_loop_step_dev(B, dx, dobst, dgoal, dX, dU, None, None, status, iters, None, flags=flags | reset, stream=st)
            torch.cuda.current_stream().synchronize()
            st_k, it_k = status.cpu().numpy(), iters.cpu().numpy()
            it_sum += it_k; failed += st_k == 4; capped += st_k == 2
        torch.cuda.current_stream().synchronize()
        got_it, got_st = iters_acc.cpu().numpy(), status_acc.cpu().numpy()
        s.set_accumulators(None, None)
    assert failed[1] == STEPS and it_sum.sum() > 0
    assert np.array_equal(got_it, it_sum)
    assert np.array_equal(got_st & 0xffff, failed) and np.array_equal(got_st >> 16, capped)
