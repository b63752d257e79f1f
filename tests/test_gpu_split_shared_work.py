"""rti_split_kernel's work that the lanes of a stage (or of a quad) share out among themselves instead of each repeating it or leaving it to the stage's
first lane: the sincos of the quadrature nodes (one node per lane of a quad in the fused plant step, two per part in the linearisation), the per-iteration
staging of H~aug_t (each part stores the words of the box variables it holds) and the closed-loop blocks [Acl c] (two columns per part).  None of it changes a
value, only the lane that forms or stores it, so every comparison is bit for bit (array_equal):
  * one fused control step == solve, plant step, obstacle step and shift through their own entry points (helpers.fused_step_is_the_separate_calls), three steps
    running, on the four shapes that differ in how the lanes are dealt: three lanes per stage at N = 20 and at N = 3 (most lanes of the wavefront hold no stage),
    two lanes per stage at N = 21 and at N = 31 (all 64 lanes are stage lanes: no idle lane behind the last stage).  The plant step of the separate side is
    plant_step_kernel, which walks the four nodes in one lane (dyn_step): this pins the bits of the dealt plant step.  The helper passes no episode buffers, so
    the bookkeeping flag (STEP_METRICS, rejected without them) is exercised by the second test;
  * the same comparison in a loop of its own, with the episode bookkeeping on, on headings that take BOTH arms of sincos's argument reduction within one call:
    the device library reduces |x| < 2^30 with the three-constant Cody-Waite form and larger arguments with the Payne-Hanek form (the listing of the kernel:
    v_cmp_nlt_f64 |x|, 0x41d0000000000000, then the v_trig_preop_f64 block).  The warm start carries stage headings of 0, pi, 1e3 and 1e12 within every instance
    (the parts of different stages take different arms in one linearisation), and the plant headings are 0.3, -pi, 1e12 and 2^30 - 0.03 with a yaw rate of 1,
    whose four nodes straddle 2^30: lanes of ONE quad take different arms in one plant step.  The minimum margin the kernel records is compared with the
    distance of the separate side's states (12 digits: the kernel contracts dx dx + dy dy into an FMA, numpy does not)."""
import numpy as np
import pytest

from helpers import ARENA, fused_step_is_the_separate_calls, wall_batch

pytestmark = pytest.mark.gpu

B, STEPS = 12, 3
R_HIT = 1.0 + 0.2       # obstacle radius + robot radius, as mpc_closed_loop_step_dev sets it


@pytest.fixture
def env(built):
    import mpc_gpu
    return mpc_gpu


def split(lps):
    def configure(s):
        s.set_lanes_per_stage(lps)
        assert s.lanes_per_stage(B) == lps and s.waves_per_simd(B) == 1
        assert "rti_split_kernel" in s.kernel_name(B)
    return configure


@pytest.mark.parametrize("lps,N,no", [(3, 20, 3), (3, 3, 1), (2, 21, 3), (2, 31, 3)])
def test_fused_step_is_the_separate_calls(env, lps, N, no):
    from mpc_gpu import _lib
    mpc_gpu = env
    x0, goal, obst = wall_batch(B, no, seed=8100 + 10 * N + lps)
    obst[3, 0] = [ARENA - 0.1, -ARENA + 0.1, 1.8, -1.8]         # a ground-truth reflection as well
    x0[:, 3] = np.linspace(-0.5, 1.5, B); x0[:, 4] = np.linspace(-1.0, 1.0, B)       # moving and turning: the four nodes differ
    noise = np.random.default_rng(81).standard_normal((STEPS, B, no, 2))
    fused = fused_step_is_the_separate_calls(mpc_gpu, N, no, x0, goal, obst, noise, split(lps),
                                             _lib.STEP_SHIFT | _lib.STEP_PLANT | _lib.STEP_OBSTACLES, steps=STEPS)
    assert (fused[-1]["status"] != 4).any()
    assert not np.array_equal(fused[-1]["x"][:, :2], x0[:, :2])


def test_both_arms_of_the_argument_reduction_in_one_call(env):
    import torch
    from mpc_gpu import _lib
    mpc_gpu = env
    lps, N, no = 3, 20, 3
    x0, goal, obst = wall_batch(B, no, seed=8300)
    x0[:, 2] = np.tile([0.3, -np.pi, 1e12, 2.0 ** 30 - 0.03], B // 4)
    x0[:, 3] = 1.0; x0[:, 4] = 1.0
    goal[:, 0] = np.where(x0[:, 0] > 0.0, -5.0, 5.0)        # out of reach in three steps: a reached goal ends the fused side's episode, not the separate calls
    assert 2.0 ** 30 - 0.03 + 0.0694 * 0.1 < 2.0 ** 30 < 2.0 ** 30 - 0.03 + 0.33 * 0.1     # nodes 0 and 1 of the plant step on either side
    heading = np.tile([0.0, np.pi, 1e3, 1e12, -1e12, -1e3, 2.0 ** 30, 0.5], 3)[:N + 1]      # per stage, within every instance
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    c = lambda a: a.cpu().numpy()

    def handle():
        s = mpc_gpu.BatchedMpc(N, no, 0.1 * N, max_batch=B)
        split(lps)(s)
        s.reset_guess(x0)
        X, U = s.get_traj(B)
        X[:, 1:, 2] = heading[1:]; X[:, 1:, 3] = 0.7; U[:, :, 1] = 0.4
        s.set_warmstart(X, U)
        return s

    flags = _lib.STEP_SHIFT | _lib.STEP_PLANT | _lib.STEP_OBSTACLES | _lib.STEP_METRICS
    fused, apart = [], []
    with handle() as s, torch.cuda.stream(torch.cuda.Stream(device=dev)):
        st = torch.cuda.current_stream().cuda_stream
        dx, dobst, dgoal = t(x0), t(obst), t(goal)
        u0 = torch.zeros(B, 2, dtype=torch.float64, device=dev); cost = torch.zeros(B, dtype=torch.float64, device=dev)
        status = torch.zeros(B, dtype=torch.int32, device=dev); iters = torch.zeros(B, dtype=torch.int32, device=dev)
        margin = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
        ep_flags = torch.zeros(B, dtype=torch.int32, device=dev); ep_steps = torch.zeros(B, dtype=torch.int32, device=dev)
        dX, dU, _ = s.iterate_ptrs()
        for k in range(STEPS):
            s.closed_loop_step_dev(B, dx, dobst, dgoal, dX, dU, u0, cost, status, iters, None, flags=flags,
                                   min_margin=margin, ep_flags=ep_flags, ep_steps=ep_steps, stream=st)
            torch.cuda.current_stream().synchronize()
            X, U = s.get_traj(B)
            fused.append(dict(X=X, U=U, x=c(dx), obst=c(dobst), u0=c(u0), cost=c(cost), status=c(status), iters=c(iters)))
        margin, ep_flags, ep_steps = c(margin), c(ep_flags), c(ep_steps)
    with handle() as s, torch.cuda.stream(torch.cuda.Stream(device=dev)):
        st = torch.cuda.current_stream().cuda_stream
        x, ob = x0.copy(), obst.copy()
        for k in range(STEPS):
            g = s.solve(x, ob, goal)
            x = s.plant_step(x, g["u0"])
            dob = t(ob)
            s.obstacle_step_dev(B * no, dob, None, stream=st)
            torch.cuda.current_stream().synchronize()
            ob = c(dob)
            s.shift(B)
            X, U = s.get_traj(B)
            apart.append(dict(X=X, U=U, x=x, obst=ob, u0=g["u0"], cost=g["cost"], status=g["status"], iters=g["iters"]))
    for k, (a, b) in enumerate(zip(fused, apart)):
        for key in ("X", "U", "x", "obst", "u0", "cost", "status", "iters"):
            assert np.array_equal(a[key], b[key]), (k, key)
    # the plant moved, on every heading, and by finite amounts
    assert np.isfinite(fused[-1]["x"]).all()
    assert (np.abs(fused[0]["x"][:, :2] - x0[:, :2]).max(axis=1) > 1e-3).all()
    # bookkeeping of the fused side against the separate side's states
    d = np.stack([np.hypot(b["x"][:, None, 0] - b["obst"][:, :, 0], b["x"][:, None, 1] - b["obst"][:, :, 1]).min(axis=1) - R_HIT for b in apart])
    assert ((ep_flags & 1) == 0).all()
    assert np.allclose(margin, d.min(axis=0), rtol=0.0, atol=1e-12)
    assert (ep_steps == STEPS).all()
