"""The GPU plumbing the per-instance feature levels' tests share (per-stage reference, instance parameters, obstacle mask, instance bounds, the
off-default sweep): the `mg` fixture, handles and repeated solves (`make`, `run`, `assert_same`), and the ONE transcription of the fused control
step's bookkeeping -- `fused_loop` (the resident fused closed loop) against `host_driven_loop` (the same steps through solve + plant_step + shift + the
obstacle kernel, the episode words in numpy), compared by `assert_fused_equals_host`.  `FeatureStack` says what is layered on the handle; a new feature
level adds a field to it, not a loop of its own.  `step_bookkeeping` is that step's episode bookkeeping in numpy, and `Banded` the guard-banded device
arrays of the every-kernel sweeps.  (tests/helpers.py is the oracle / QP side.)  torch is imported inside the functions only."""
import dataclasses

import numpy as np
import pytest

OWN_ARGS = {"rti_solve_kernel": 4, "rti_split_kernel": 5, "rti_wide_kernel": 3}      # template arguments in front of the feature levels


def reset_mapping_defaults(mpc_gpu):
    mpc_gpu.BatchedMpc.default_lanes_per_stage = 0
    mpc_gpu.BatchedMpc.default_waves_per_simd = 0
    mpc_gpu.BatchedMpc.default_lanes_per_instance = 0


@pytest.fixture
def mg(built):
    import mpc_gpu
    from oracle import oracle as orc
    reset_mapping_defaults(mpc_gpu)
    return mpc_gpu, orc


def on_own_stream(fn, *args):
    """device-API calls on a torch stream of their own: the legacy default stream's handle is 0, which the library reads as the handle's
    own (non-blocking) stream, unordered with torch's copies"""
    import torch
    with torch.cuda.stream(torch.cuda.Stream()):
        fn(*args)
        torch.cuda.synchronize()


def make(mpc_gpu, N, no, B, scheduling=False, **cfg):
    """scheduling False: the launch order depends on nothing but the batch; True: the handle's default, instance scheduling on"""
    s = mpc_gpu.BatchedMpc(N, no, 0.1 * N, max_batch=B, **cfg)
    if not scheduling:
        s.set_instance_scheduling(False)
    return s


_SCHEDULED = {}
SCHEDULED_LIMIT = 2048


def smallest_scheduled_batch(mpc_gpu, N=20, no=3, configure=None, key=None, limit=SCHEDULED_LIMIT):
    """the first batch size, in steps of half the device's compute-unit count (+ 13, so that the last wavefront is partly empty), after whose first
    launch instance_order is not None: the scheduler deals batches beyond one wavefront per SIMD, and how many SIMDs the device has is the library's
    knowledge, not the test's.  configure(s): the lane mapping of the handles asked (`key` names it); found once per (N, no, key) and session"""
    import torch
    from helpers import random_batch
    if (N, no, key) not in _SCHEDULED:
        step = max(1, torch.cuda.get_device_properties(0).multi_processor_count // 2)
        x0, goal, obst = random_batch(limit, no, seed=100 + N + no)
        found = None
        for B in range(step + 13, limit + 1, step):
            with mpc_gpu.BatchedMpc(N, no, 0.1 * N, max_batch=B) as s:
                if configure is not None:
                    configure(s)
                s.set_instance_scheduling(True)
                s.reset_guess(x0[:B])
                s.solve(x0[:B], obst[:B], goal[:B])
                if s.instance_order(B) is not None:
                    found = B
                    break
        assert found is not None, f"no batch up to {limit} is dealt by the instance scheduler"
        _SCHEDULED[N, no, key] = found
    return _SCHEDULED[N, no, key]


def run(s, x0, obst, goal, steps=3):
    """first solve and warm-started ones; everything a caller sees"""
    B = x0.shape[0]
    s.reset_guess(x0)
    outs = []
    for _ in range(steps):
        o = s.solve(x0, obst, goal)
        X, U = s.get_traj(B)
        outs.append((X, U, o["u0"], o["cost"], o["status"], o["iters"]))
    return outs


def assert_same(a, b, rows_a=None, rows_b=None, cost_rtol=None):
    """two `run` results: X, U, u0, status, iterations bit for bit; the reported cost bit for bit too, or to cost_rtol when one is given.
    rows_a / rows_b: the instances of `a` / `b` that are compared"""
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        for k, (x, y) in enumerate(zip(ra, rb)):
            x = x if rows_a is None else x[rows_a]
            y = y if rows_b is None else y[rows_b]
            if k == 3 and cost_rtol is not None:
                assert np.allclose(x, y, rtol=cost_rtol, atol=0.0), (x, y)
            else:
                assert np.array_equal(x, y), k


def cfg_values(s):
    return np.array([s.cfg.W[k] for k in range(6)]), np.array([s.cfg.We[k] for k in range(4)]), float(s.cfg.r_safe)


def level_of(name):
    """feature level of a kernel name: the `, true` behind the family's own template arguments (whose last may be `true` itself: MASKED)"""
    family, args = name.rstrip(">").split("<")
    args = args.split(", ")
    assert all(a == "true" for a in args[OWN_ARGS[family]:]), name
    return len(args) - OWN_ARGS[family]


def smooth_path(rng, B, T):
    """random smooth reference paths with non-zero v / omega / input rows"""
    t = np.linspace(0.0, 1.0, T)
    R = np.zeros((B, T, 6))
    for b in range(B):
        a = rng.uniform(-4, 4, 2); c = rng.uniform(-3, 3, 2); w = rng.uniform(0.5, 2.0)
        R[b, :, 0] = a[0] + c[0] * np.sin(w * t); R[b, :, 1] = a[1] + c[1] * np.cos(w * t)
        R[b, :, 2] = rng.uniform(-1, 1) + 0.3 * t; R[b, :, 3] = rng.uniform(-0.5, 0.5) * np.cos(t)
        R[b, :, 4] = rng.uniform(-0.5, 0.5); R[b, :, 5] = rng.uniform(-0.3, 0.3)
    return R


GUARD = 64           # sentinel words on either side of every array of a Banded buffer


class Banded:
    """device arrays carved out of one sentinel-filled buffer"""

    def __init__(self, torch, dev):
        self.torch, self.dev, self.items = torch, dev, []

    def f64(self, *shape, init=0.0):
        t = self.torch.full((int(np.prod(shape)) + 2 * GUARD,), -7.25e77, dtype=self.torch.float64, device=self.dev)
        v = t[GUARD:-GUARD].view(*shape); v.fill_(init); self.items.append((t, "f64")); return v

    def i32(self, *shape, init=0):
        t = self.torch.full((int(np.prod(shape)) + 2 * GUARD,), -1234567, dtype=self.torch.int32, device=self.dev)
        v = t[GUARD:-GUARD].view(*shape); v.fill_(init); self.items.append((t, "i32")); return v

    def intact(self):
        for t, kind in self.items:
            s = -7.25e77 if kind == "f64" else -1234567
            if not (bool((t[:GUARD] == s).all()) and bool((t[-GUARD:] == s).all())):
                return False
        return True


# ---------------------------------------------------------------------------------------------------------------- the fused loop and its transcription
@dataclasses.dataclass
class FeatureStack:
    """what is layered on a handle; None: not set.  `mask` (bool (B, n_obst)) and `bounds` (the keywords of set_instance_bounds) given as a pair
    (first, second) switch from the first to the second at step steps // 2; given alone they hold for the whole loop."""
    W: object = None            # (B, 6)
    We: object = None           # (B, 4)
    r_safe: object = None       # (B, n_obst)
    mask: object = None
    bounds: object = None
    path: object = None         # the reference (B, T, 6), its window advancing with every step

    def instance_params(self):
        return {k: v for k, v in (("W", self.W), ("We", self.We), ("r_safe", self.r_safe)) if v is not None}


def _halves(v):
    return v if isinstance(v, tuple) else (v, None)


def fused_loop(mpc_gpu, N, no, B, steps, x0, goal, obst, stack, solver=None, handle=None):
    """`steps` fused steps, everything resident; the mask words and the packed bounds are device tensors, rewritten by a torch op halfway through
    where the stack gives a pair.  `solver`: a PipelinedMpc, which takes everything as device tensors through its *_dev setters.  `handle`: a
    BatchedMpc of the caller's (its instance scheduling as the caller set it), which stays open; neither: a fresh unscheduled handle."""
    import torch
    L = mpc_gpu._lib
    dev = torch.device("cuda", 0)
    tt = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)
    s = solver or handle or make(mpc_gpu, N, no, B)
    piped = solver is not None
    tx, to, tg = tt(x0), tt(obst), tt(goal)
    X = torch.zeros((B, N + 1, 5), dtype=torch.float64, device=dev); U = torch.zeros((B, N, 2), dtype=torch.float64, device=dev)
    u0 = torch.zeros((B, 2), dtype=torch.float64, device=dev)
    mm = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
    fl = torch.zeros(B, dtype=torch.int32, device=dev); ns = torch.zeros(B, dtype=torch.int32, device=dev)
    flags = L.STEP_SHIFT | L.STEP_PLANT | L.STEP_OBSTACLES | L.STEP_METRICS
    switch = []                 # (the tensor the handle reads in place, what it holds from halfway on)
    if stack.bounds is not None:
        b1, b2 = _halves(stack.bounds)
        table = tt(mpc_gpu.pack_instance_bounds(s.cfg, B, **b1))
        if b2 is not None:
            switch.append((table, tt(mpc_gpu.pack_instance_bounds(s.cfg, B, **b2))))
        s.set_instance_bounds_dev(table)
    if stack.mask is not None:
        act1, act2 = _halves(stack.mask)
        words = tt(mpc_gpu.pack_obstacle_mask(act1).view(np.int32))
        if act2 is not None:
            switch.append((words, tt(mpc_gpu.pack_obstacle_mask(act2).view(np.int32))))
        if piped:
            s.set_obstacle_mask_dev(words)
        else:
            s.set_obstacle_mask(words)
    par = stack.instance_params()
    if par:
        dpar = {k: tt(v) for k, v in par.items()}
        if piped:
            s.set_instance_params_dev(**dpar)
        elif stack.W is None:
            s.set_instance_params(**dpar)       # radii on top of a mask: the device form on the plain handle too
        else:
            s.set_instance_params(**par)        # whole parameter sets: host arrays, which the pipelined run's device arrays are compared with
    if stack.path is not None:
        ty, toff = tt(stack.path), torch.zeros(B, dtype=torch.int32, device=dev)
        if piped:
            s.set_reference_dev(ty, toff)
        else:
            s.set_reference(ty, toff)
        flags |= L.STEP_ADVANCE_REF
    us = []
    torch.cuda.synchronize()
    kw = {} if piped else dict(stream=torch.cuda.current_stream().cuda_stream)
    if stack.bounds is not None:
        assert level_of(s.kernel_name(B)) == 4
    s.reset_guess_dev(B, tx, X, U, **kw)
    for k in range(steps):
        if k == steps // 2 and switch:
            torch.cuda.synchronize()
            for held, second in switch:
                held.copy_(second)       # a torch op, no library call
            torch.cuda.synchronize()
        s.closed_loop_step_dev(B, tx, to, tg, X, U, u0, flags=flags, min_margin=mm, ep_flags=fl, ep_steps=ns, **kw)
        if piped:
            for _, _, _, ps in s.parts:
                ps.synchronize()
        torch.cuda.synchronize()
        us.append(u0.cpu().numpy().copy())
    res = dict(x=tx.cpu().numpy(), obst=to.cpu().numpy(), X=X.cpu().numpy(), U=U.cpu().numpy(), u0=np.array(us), mm=mm.cpu().numpy(),
               fl=fl.cpu().numpy(), ns=ns.cpu().numpy())
    if solver is None and handle is None:
        s.close()
    return res


def step_bookkeeping(x, ob, goal, act, r_hit, arena, alive, mm, fl, ns):
    """The episode bookkeeping of one fused step in numpy, on the state after the plant step and the obstacle motion: the running minimum margin over the
    present obstacles (act (B, n_obst); r_hit (B, n_obst)), the arena, hit and goal flags and the step counters, updated in place for the instances
    `alive` alone.  Returns which instances are within the goal tolerance."""
    dist = np.linalg.norm(x[:, None, :2] - ob[:, :, :2], axis=2) - r_hit
    margin = np.where(act, dist, np.inf).min(axis=1)
    mm[alive] = np.minimum(mm, margin)[alive]
    a_ = x[:, 0]; b_ = x[:, 1]
    fl[alive & ((a_ < arena[0]) | (a_ > arena[1]) | (b_ < arena[2]) | (b_ > arena[3]))] |= 2
    fl[alive & (mm <= 0.0)] |= 4
    reached = np.linalg.norm(x[:, :2] - goal, axis=1) <= 0.15
    fl[alive & reached] |= 1
    ns[alive & ~reached] += 1
    return reached


def host_driven_loop(mpc_gpu, N, no, B, steps, x0, goal, obst, stack):
    """the same steps through mpc_solve_obst + mpc_plant_step + mpc_shift (and the obstacle motion kernel), a mask or bounds that switch set through
    the host setters at the same step, the bookkeeping in numpy over the present obstacles: an instance that has reached its goal idles, nothing of
    it is touched"""
    import torch
    dev = torch.device("cuda", 0)
    x, ob = x0.copy(), obst.copy()
    alive = np.ones(B, bool)
    mm = np.full(B, np.inf); ns = np.zeros(B, np.int32); fl = np.zeros(B, np.int32)
    us, u_last = [], np.zeros((B, 2))
    off = np.zeros(B, np.int32)
    r_hit = np.full((B, no), 1.2) if stack.r_safe is None else stack.r_safe - (2.4 - 1.2)
    act = np.ones((B, no), bool)
    with make(mpc_gpu, N, no, B) as s:
        if stack.instance_params():
            s.set_instance_params(**stack.instance_params())
        if stack.mask is not None and not isinstance(stack.mask, tuple):
            act = stack.mask
            s.set_obstacle_mask(act)
        s.reset_guess(x)
        ar = [float(v) for v in s.cfg.arena]
        for k in range(steps):
            half = int(k >= steps // 2)
            if isinstance(stack.mask, tuple):
                act = stack.mask[half]
                s.set_obstacle_mask(act)
            if stack.bounds is not None:
                s.set_instance_bounds(**(stack.bounds[half] if isinstance(stack.bounds, tuple) else stack.bounds))
            Xk, Uk = s.get_traj(B)
            if stack.path is not None:
                s.set_reference(stack.path, offset=off)
            o = s.solve(x, ob, goal)
            xn = s.plant_step(x, o["u0"])
            s.shift(B)
            Xn, Un = s.get_traj(B)
            to = torch.tensor(ob, device=dev)
            s.obstacle_step_dev(B * no, to, None, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            obn = to.cpu().numpy()
            Xn[~alive] = Xk[~alive]; Un[~alive] = Uk[~alive]
            s.set_warmstart(Xn, Un)
            x[alive] = xn[alive]; ob[alive] = obn[alive]; u_last[alive] = o["u0"][alive]
            off[alive] += 1
            alive &= ~step_bookkeeping(x, ob, goal, act, r_hit, ar, alive, mm, fl, ns)
            us.append(u_last.copy())
        X, U = s.get_traj(B)
    return dict(x=x, obst=ob, X=X, U=U, u0=np.array(us), mm=mm, ns=ns, fl=fl)


def assert_fused_equals_host(f, h):
    for k in ("x", "obst", "X", "U", "u0", "ns"):
        assert np.array_equal(f[k], h[k]), k
    both = np.isfinite(h["mm"])
    assert np.array_equal(np.isfinite(f["mm"]), both)
    assert np.abs(f["mm"][both] - h["mm"][both]).max(initial=0.0) <= 1e-12      # (numpy's norm against the kernel's sqrt of a contracted sum)
    margin_clear = np.abs(h["mm"]) > 1e-9
    assert np.array_equal(f["fl"][margin_clear], h["fl"][margin_clear])


def resident_steps(mpc_gpu, s, B, N, x0, goal, obst, steps, noise=None, extra_flags=0):
    """`steps` fused steps of the handle `s` as it stands, with velocity noise (steps, B, n_obst, 2) if given: u0, cost, x and obst after every step,
    the last iterate and the episode words"""
    import torch
    L = mpc_gpu._lib
    dev = torch.device("cuda", 0)
    tt = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)
    tx, to, tg = tt(x0), tt(obst), tt(goal)
    tn = None if noise is None else tt(noise)
    X = torch.zeros((B, N + 1, 5), dtype=torch.float64, device=dev); U = torch.zeros((B, N, 2), dtype=torch.float64, device=dev)
    u0 = torch.zeros((B, 2), dtype=torch.float64, device=dev); cost = torch.zeros(B, dtype=torch.float64, device=dev)
    mm = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
    fl = torch.zeros(B, dtype=torch.int32, device=dev); ns = torch.zeros(B, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    s.reset_guess_dev(B, tx, X, U, stream=st)
    us, cs, xs, os_ = [], [], [], []
    for k in range(steps):
        s.closed_loop_step_dev(B, tx, to, tg, X, U, u0, cost, noise=None if tn is None else tn[k],
                               flags=L.STEP_SHIFT | L.STEP_PLANT | L.STEP_OBSTACLES | L.STEP_METRICS | extra_flags,
                               min_margin=mm, ep_flags=fl, ep_steps=ns, stream=st)
        torch.cuda.synchronize()
        us.append(u0.cpu().numpy().copy()); cs.append(cost.cpu().numpy().copy()); xs.append(tx.cpu().numpy().copy()); os_.append(to.cpu().numpy().copy())
    return dict(u0=np.array(us), cost=np.array(cs), x=np.array(xs), obst=np.array(os_), X=X.cpu().numpy(), U=U.cpu().numpy(), mm=mm.cpu().numpy(), fl=fl.cpu().numpy())


class GpuLoop:
    """device-resident closed loop on the handle-owned iterate, one launch per control step"""

    def __init__(self, mpc_gpu, N, no, Tf, x0, goal, obst, alias=True, **cfg):
        import torch
        from mpc_gpu import _lib
        self.torch, self.B = torch, x0.shape[0]
        self.m = mpc_gpu.BatchedMpc(N, no, Tf, max_batch=self.B, **cfg)
        dev = torch.device("cuda:0")
        self.stream = torch.cuda.Stream(device=dev)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
        z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=dev)
        with torch.cuda.stream(self.stream):
            self.x0, self.goal, self.obst = t(x0), t(goal), t(obst)
            if alias:
                self.x0[:, 3:] = 0.0
            self.u0, self.cost = z(self.B, 2), z(self.B)
            self.status, self.iters = z(self.B, dt=torch.int32), z(self.B, dt=torch.int32)
            self.margin = torch.full((self.B,), float("inf"), dtype=torch.float64, device=dev)
            self.flags, self.steps = z(self.B, dt=torch.int32), z(self.B, dt=torch.int32)
        self.stream.synchronize()
        self.dX, self.dU, _ = self.m.iterate_ptrs()              # the handle-owned iterate: terminal_state() / get_traj() see it
        self.m.reset_guess_dev(self.B, self.x0, self.dX, self.dU, stream=self.stream.cuda_stream)
        self.fl = (_lib.STEP_SHIFT | _lib.STEP_PLANT | _lib.STEP_OBSTACLES | _lib.STEP_METRICS | _lib.STEP_RESET_ON_FAIL
                   | (_lib.STEP_ALIAS_BUG if alias else 0))
        self.dev = dev

    def step(self, noise=None):
        nz = None if noise is None else self.torch.from_numpy(np.ascontiguousarray(noise)).to(self.dev)
        self.m.closed_loop_step_dev(self.B, self.x0, self.obst, self.goal, self.dX, self.dU, self.u0, self.cost, self.status, self.iters,
                                    nz, flags=self.fl, min_margin=self.margin, ep_flags=self.flags, ep_steps=self.steps,
                                    stream=self.stream.cuda_stream)
        self.stream.synchronize()

    def host(self):
        c = lambda a: a.cpu().numpy()
        X, U = self.m.get_traj(self.B)
        return dict(x0=c(self.x0), obst=c(self.obst), X=X, U=U, u0=c(self.u0), status=c(self.status), iters=c(self.iters),
                    margin=c(self.margin), flags=c(self.flags), steps=c(self.steps))

    def set_goal(self, goal):
        with self.torch.cuda.stream(self.stream):
            self.goal.copy_(self.torch.from_numpy(np.ascontiguousarray(goal)).to(self.dev))
        self.stream.synchronize()

    def close(self):
        self.m.close()
