"""The work of rti_split_kernel around its interior-point loop: the look-ahead walk (four stages per exit test away from the walls), the obstacle
motion of the fused step (advanced in front of the loop and parked in the look-ahead's staging region), the epilogue's grouped loads and stores.
Every comparison is bit for bit (array_equal): nothing here changes arithmetic, only where and when it runs.
  * look-ahead in the kernel == the positions predict_kernel gives for the same states, with obstacles that reflect inside the horizon and one
    that starts exactly on a wall (a walking lane's store landing in a live word; a block of four stages walked one stage off);
  * one fused control step == solve, plant step, obstacle step and shift through their own entry points, three steps running, with and without
    velocity noise, both wavefront variants (a parked obstacle state read before the look-ahead is done with the region; stores out of order);
  * a NaN in one instance's obstacle states fails that instance (status 4) and leaves its neighbours untouched (the finiteness sum)."""
import numpy as np
import pytest

from helpers import ARENA, fused_step_is_the_separate_calls, wall_batch

pytestmark = pytest.mark.gpu


@pytest.fixture
def env(built):
    import mpc_gpu
    return mpc_gpu


def lanes_for(N):
    return 3 if N <= 20 else 2


@pytest.mark.parametrize("N,no", [(5, 1), (5, 3), (20, 3), (20, 5), (21, 10)])
def test_lookahead_in_the_kernel_is_the_lookahead_given(env, N, no):
    mpc_gpu = env
    B = 3
    x0, goal, obst = wall_batch(B, no, seed=4100 + 10 * N + no)
    res = {}
    for how in ("obst", "P"):
        with mpc_gpu.BatchedMpc(N, no, 0.1 * N, max_batch=B) as s:
            s.set_lanes_per_stage(lanes_for(N))
            assert s.lanes_per_stage(B) == lanes_for(N)
            P = s.predict(obst)
            if how == "P":
                # the walls are met inside the horizon: some coordinate does not move monotonically, and one starts on the wall
                d = np.diff(P, axis=1)
                assert ((d.max(axis=1) > 0) & (d.min(axis=1) < 0)).any(), "no reflection inside the horizon"
                assert (np.abs(P[:, 0]) == ARENA).any()
            s.reset_guess(x0)
            g = s.solve(x0, obst if how == "obst" else P, goal)
            X, U = s.get_traj(B)
            res[how] = (g, X, U)
    (ga, Xa, Ua), (gb, Xb, Ub) = res["obst"], res["P"]
    assert np.array_equal(Xa, Xb) and np.array_equal(Ua, Ub)
    for key in ("u0", "cost", "status", "iters"):
        assert np.array_equal(ga[key], gb[key]), key
    assert (ga["status"] != 4).any()


@pytest.mark.parametrize("waves", [1, 2])
@pytest.mark.parametrize("noisy", [False, True], ids=["no-noise", "noise"])
@pytest.mark.parametrize("N,no", [(5, 3), (20, 3)])
def test_fused_step_is_the_separate_calls(env, N, no, noisy, waves):
    from mpc_gpu import _lib
    mpc_gpu = env
    B, steps = 5, 3
    x0, goal, obst = wall_batch(B, no, seed=5200 + N)
    # ground-truth reflections as well: the step moves x with vx
    obst[3, 0] = [ARENA - 0.1, -ARENA + 0.1, 1.8, -1.8]
    noise = np.random.default_rng(77).standard_normal((steps, B, no, 2)) if noisy else None

    def configure(s):
        s.set_lanes_per_stage(3); s.set_waves_per_simd(waves)
        assert s.lanes_per_stage(B) == 3 and s.waves_per_simd(B) == waves

    fused_step_is_the_separate_calls(mpc_gpu, N, no, x0, goal, obst, noise, configure, _lib.STEP_SHIFT | _lib.STEP_PLANT | _lib.STEP_OBSTACLES, steps=steps)


def test_a_nan_obstacle_fails_its_instance_alone(env):
    mpc_gpu = env
    N, no, B = 20, 3, 3
    x0, goal, obst = wall_batch(B, no, seed=6300)
    bad = obst.copy(); bad[1, 2, 1] = np.nan
    res = {}
    for name, ob in (("clean", obst), ("nan", bad)):
        with mpc_gpu.BatchedMpc(N, no, 0.1 * N, max_batch=B) as s:
            s.set_lanes_per_stage(3)
            s.reset_guess(x0)
            X0, U0 = s.get_traj(B)
            g = s.solve(x0, ob, goal)
            res[name] = (g, *s.get_traj(B))
    (gc, Xc, Uc), (gn, Xn, Un) = res["clean"], res["nan"]
    assert gn["status"][1] == 4
    assert np.array_equal(Xn[1], X0[1]) and np.array_equal(Un[1], U0[1])       # a failed instance keeps its iterate
    for b in (0, 2):
        assert gc["status"][b] != 4
        assert np.array_equal(Xn[b], Xc[b]) and np.array_equal(Un[b], Uc[b])
        for key in ("u0", "cost", "status", "iters"):
            assert np.array_equal(gn[key][b], gc[key][b]), (b, key)
