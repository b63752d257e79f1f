"""Per-instance box bounds (mpc_set_instance_bounds, BatchedMpc.set_instance_bounds, PipelinedMpc.set_instance_bounds_dev) on the GPU: uniform bounds are
the configured handle bit for bit on all eleven instantiations, a mixed batch is its groups bit for bit, mixed bounds are judged against the oracle
group by group, the fused loop equals host-driven steps with the table rewritten on the device, pipelined sub-batches equal one handle, the refusals
and switching off, and run_episodes."""
import numpy as np
import pytest

from helpers import allowed_adjudications, judge_against_oracle, oracle_P, oracle_reference, random_batch
from instance_bounds_cases import DEFAULTS, as_cfg, draw_bounds, per_instance
from obstacle_mask_cases import draw_masks

pytestmark = pytest.mark.gpu

# split x3 / split x2 on 3, 5, 10 rows; one instance per wavefront on 3, 5, 10 rows; the multi-wavefront kernel on 20 and 32 rows: the eleven instantiations
ALL_SIZES = [(20, 3), (30, 3), (20, 5), (30, 5), (20, 10), (30, 10), (50, 3), (50, 5), (50, 10), (20, 15), (20, 25)]
LEVEL4 = ", true, true, true, true>"
OWN_ARGS = {"rti_solve_kernel": 4, "rti_split_kernel": 5, "rti_wide_kernel": 3}      # template arguments in front of the feature levels


def level_of(name):
    """feature level of a kernel name: the `, true` behind the family's own template arguments (whose last may be `true` itself: MASKED)"""
    family, args = name.rstrip(">").split("<")
    args = args.split(", ")
    assert all(a == "true" for a in args[OWN_ARGS[family]:]), name
    return len(args) - OWN_ARGS[family]


@pytest.fixture
def mg(built):
    import mpc_gpu
    from oracle import oracle as orc
    mpc_gpu.BatchedMpc.default_lanes_per_stage = 0
    mpc_gpu.BatchedMpc.default_waves_per_simd = 0
    mpc_gpu.BatchedMpc.default_lanes_per_instance = 0
    return mpc_gpu, orc


def _on_own_stream(fn, *args):
    """device-API calls on a torch stream of their own: the legacy default stream's handle is 0, which the library reads as the handle's
    own (non-blocking) stream, unordered with torch's copies"""
    import torch
    with torch.cuda.stream(torch.cuda.Stream()):
        fn(*args)
        torch.cuda.synchronize()


def make(mpc_gpu, N, no, B, **cfg):
    s = mpc_gpu.BatchedMpc(N, no, 0.1 * N, max_batch=B, **cfg)
    s.set_instance_scheduling(False)      # (the launch order then depends on nothing but the batch)
    return s


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


def assert_same(a, b, rows_a=None, rows_b=None):
    """X, U, u0, cost, status, iterations bit for bit (of the given instances)"""
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        for k, (x, y) in enumerate(zip(ra, rb)):
            x = x if rows_a is None else x[rows_a]
            y = y if rows_b is None else y[rows_b]
            assert np.array_equal(x, y), k


def tiled(entry, B):
    return {k: np.tile(v, (B, 1)) for k, v in entry.items()}


# ---------------------------------------------------------------------------------------------------------------- 1. uniform bounds are the configured handle
def _body_uniform(mg, N, no):
    mpc_gpu, orc = mg
    B = 8
    x0, goal, obst = random_batch(B, no, seed=17 * N + no + B)
    x0[:, 3:] = 0.0
    entry = draw_bounds(np.random.default_rng(50 + N + no), B)[0][1]
    P = oracle_P(orc, orc.config(N, no, 0.1 * N), obst)
    for what, e, cfg in (("non-default", entry, as_cfg(entry)), ("defaults", DEFAULTS, {})):
        with make(mpc_gpu, N, no, B, **cfg) as a, make(mpc_gpu, N, no, B) as b:
            a.set_obstacle_mask(np.ones((B, no), bool))
            b.set_instance_bounds(**tiled(e, B))
            name = b.kernel_name(B)
            print(N, no, what, "bounds:", name, "| configured:", a.kernel_name(B))
            assert name.endswith(LEVEL4) and level_of(name) == 4, name
            assert level_of(a.kernel_name(B)) == 3
            assert name.split("<")[0] == a.kernel_name(B).split("<")[0]                  # the same family
            assert name == a.kernel_name(B)[:-1] + ", true>"                             # ... and the same instantiation of it, one level up
            ra, rb = run(a, x0, obst, goal), run(b, x0, obst, goal)                      # look-ahead in the kernel
            assert_same(ra, rb)
            assert_same(run(a, x0, P, goal, 2), run(b, x0, P, goal, 2))                  # explicit P
            assert (ra[0][4] != 4).any()                                                 # (something was solved)


@pytest.mark.parametrize("N,no", ALL_SIZES)
def test_uniform_bounds_are_the_configured_handle(mg, N, no):
    _on_own_stream(_body_uniform, mg, N, no)


# ---------------------------------------------------------------------------------------------------------------- 2. a mixed batch is its groups
def _body_groups(mg, N, no):
    mpc_gpu, _ = mg
    B = 16
    x0, goal, obst = random_batch(B, no, seed=23 * N + no)
    x0[:, 3:] = 0.0
    menu, group = draw_bounds(np.random.default_rng(300 + N + no), B)
    with make(mpc_gpu, N, no, B) as s:
        s.set_instance_bounds(**per_instance(menu, group))
        assert level_of(s.kernel_name(B)) == 4
        mixed = run(s, x0, obst, goal)
    for g, entry in enumerate(menu):
        idx = np.nonzero(group == g)[0]
        with make(mpc_gpu, N, no, len(idx), **as_cfg(entry)) as r:
            r.set_obstacle_mask(np.ones((len(idx), no), bool))
            assert level_of(r.kernel_name(len(idx))) == 3
            assert_same(mixed, run(r, x0[idx], obst[idx], goal[idx]), rows_a=idx)


@pytest.mark.parametrize("N,no", [(20, 3), (30, 10), (20, 15), (50, 10)])
def test_mixed_batch_is_its_groups(mg, N, no):
    _on_own_stream(_body_groups, mg, N, no)


# ---------------------------------------------------------------------------------------------------------------- 3. mixed bounds against the oracle
# (N, n_obst, B, seed of random_batch, bx_terminal): checked on the CPU before the first GPU run -- the oracle alone returns status 0 for every instance on
# three consecutive solves (the counts are in DESIGN.md section 4e)
ORACLE_CASES = [(20, 3, 16, 31, 0), (20, 5, 16, 32, 0), (30, 10, 16, 36, 0), (20, 15, 16, 34, 0), (50, 10, 16, 35, 0), (2, 1, 8, 5, 0), (20, 3, 16, 31, 1)]


def oracle_inputs(N, no, B, seed):
    x0, goal, obst = random_batch(B, no, seed=seed)
    x0[:, 3:] = 0.0
    menu, group = draw_bounds(np.random.default_rng(1200 + N + no), B)
    return x0, goal, obst, menu, group


def _body_oracle(mg, N, no, B, seed, bx_terminal):
    mpc_gpu, orc = mg
    x0, goal, obst, menu, group = oracle_inputs(N, no, B, seed)
    arr = per_instance(menu, group)
    cfg = orc.config(N, no, 0.1 * N)
    P = oracle_P(orc, cfg, obst)
    kw = dict(bx_terminal=1) if bx_terminal else {}
    with make(mpc_gpu, N, no, B, **kw) as s:
        thr0 = float(s.cfg.thr0)
        s.reset_guess(x0)
        X0, U0 = s.get_traj(B)
        s.solve(x0, P, goal)                                        # the default-bounds solve of the same inputs
        Xp, Up = s.get_traj(B)
        s.set_instance_bounds(**arr)
        s.reset_guess(x0)
        g1 = s.solve(x0, P, goal)
        X1, U1 = s.get_traj(B)
        g2 = s.solve(x0, P, goal)
        X2, U2 = s.get_traj(B)
    for (g, Xs, Us, Xg, Ug, which) in ((g1, X0, U0, X1, U1, "first"), (g2, X1, U1, X2, U2, "second")):      # from the reset guess, then from the GPU's own iterate
        judged = 0
        for k, entry in enumerate(menu):
            idx = np.nonzero(group == k)[0]
            cfg_k = orc.config(N, no, 0.1 * N, thr0=thr0, **as_cfg(entry), **kw)
            o = oracle_reference(orc, cfg_k, x0[idx], P[idx], goal[idx], Xs[idx], Us[idx])
            gb = {name: v[idx] for name, v in g.items()}
            n = judge_against_oracle(orc, cfg_k, x0[idx], P[idx], goal[idx], Xs[idx], Us[idx], gb, Xg[idx], Ug[idx], o)
            print(f"N {N} no {no} bx_terminal {bx_terminal}: {which} solve, group {k} ({len(idx)} instances): {n}")
            judged += n["judged_by_qp"]
        assert judged <= allowed_adjudications(cfg, B), judged      # the project's bound holds over the batch, not per group
        ok = g["status"] == 0
        print(f"N {N} no {no}: {which} solve, status 0 in {int(ok.sum())} of {B}")
        # a converged instance lies inside its OWN box: inputs of every stage, v and omega of stages 1 .. N - 1
        for b in np.nonzero(ok)[0]:
            assert (Ug[b] >= arr["bu_lo"][b] - 1e-8).all() and (Ug[b] <= arr["bu_hi"][b] + 1e-8).all(), b
            vw = Xg[b, 1:N, 3:5]
            assert (vw >= arr["bx_lo"][b, 2:] - 1e-8).all() and (vw <= arr["bx_hi"][b, 2:] + 1e-8).all(), b
    own = np.nonzero(group != 0)[0]
    differs = int((np.abs(U1[own] - Up[own]).reshape(len(own), -1).max(axis=1) > 1e-3).sum())
    print(f"N {N} no {no}: {differs} of {len(own)} instances with bounds of their own differ from the default-bounds solve")
    if N > 2:
        assert 2 * differs >= len(own), (differs, len(own))     # the bounds reached the solve


@pytest.mark.parametrize("N,no,B,seed,bx_terminal", ORACLE_CASES)
def test_mixed_bounds_against_the_oracle(mg, N, no, B, seed, bx_terminal):
    _on_own_stream(_body_oracle, mg, N, no, B, seed, bx_terminal)


# ---------------------------------------------------------------------------------------------------------------- 4. fused loop = host-driven steps
def smooth_path(rng, B, T):
    t = np.linspace(0.0, 1.0, T)
    R = np.zeros((B, T, 6))
    for b in range(B):
        a = rng.uniform(-4, 4, 2); c = rng.uniform(-3, 3, 2); w = rng.uniform(0.5, 2.0)
        R[b, :, 0] = a[0] + c[0] * np.sin(w * t); R[b, :, 1] = a[1] + c[1] * np.cos(w * t)
        R[b, :, 2] = rng.uniform(-1, 1) + 0.3 * t; R[b, :, 3] = rng.uniform(-0.5, 0.5) * np.cos(t)
        R[b, :, 4] = rng.uniform(-0.5, 0.5); R[b, :, 5] = rng.uniform(-0.3, 0.3)
    return R


def loop_inputs(N, no, B, seed, steps, extras):
    rng = np.random.default_rng(seed)
    x0, goal, obst = random_batch(B, no, seed=seed)
    x0[:, 3:] = 0.0
    act = draw_masks(rng, B, no)
    b1, b2 = per_instance(*draw_bounds(rng, B)), per_instance(*draw_bounds(rng, B))
    R = rng.uniform(1.6, 3.0, (B, no)) if extras else None
    path = smooth_path(rng, B, steps + N + 1) if extras else None
    return x0, goal, obst, act, b1, b2, R, path


def _fused(mpc_gpu, N, no, B, steps, x0, goal, obst, act, b1, b2, R, path, solver=None):
    """`steps` fused steps, everything resident, the packed bounds a device tensor rewritten by a torch op halfway through"""
    import torch
    L = mpc_gpu._lib
    dev = torch.device("cuda", 0)
    tt = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)
    s = solver or make(mpc_gpu, N, no, B)
    piped = solver is not None
    tx, to, tg = tt(x0), tt(obst), tt(goal)
    X = torch.zeros((B, N + 1, 5), dtype=torch.float64, device=dev); U = torch.zeros((B, N, 2), dtype=torch.float64, device=dev)
    u0 = torch.zeros((B, 2), dtype=torch.float64, device=dev)
    mm = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
    fl = torch.zeros(B, dtype=torch.int32, device=dev); ns = torch.zeros(B, dtype=torch.int32, device=dev)
    flags = L.STEP_SHIFT | L.STEP_PLANT | L.STEP_OBSTACLES | L.STEP_METRICS
    t1, t2 = tt(mpc_gpu.pack_instance_bounds(s.cfg, B, **b1)), tt(mpc_gpu.pack_instance_bounds(s.cfg, B, **b2))
    table = t1.clone()
    s.set_instance_bounds_dev(table)
    words = tt(mpc_gpu.pack_obstacle_mask(act).view(np.int32))
    if piped:
        s.set_obstacle_mask_dev(words)
    else:
        s.set_obstacle_mask(words)
    if R is not None:
        dR = tt(R)
        if piped:
            s.set_instance_params_dev(r_safe=dR)
        else:
            s.set_instance_params(r_safe=dR)
    if path is not None:
        ty, toff = tt(path), torch.zeros(B, dtype=torch.int32, device=dev)
        if piped:
            s.set_reference_dev(ty, toff)
        else:
            s.set_reference(ty, toff)
        flags |= L.STEP_ADVANCE_REF
    us = []
    torch.cuda.synchronize()
    st = None if piped else torch.cuda.current_stream().cuda_stream
    kw = {} if piped else dict(stream=st)
    assert level_of(s.kernel_name(B)) == 4
    s.reset_guess_dev(B, tx, X, U, **kw)
    for k in range(steps):
        if k == steps // 2:
            torch.cuda.synchronize()
            table.copy_(t2)              # a torch op, no library call
            torch.cuda.synchronize()
        s.closed_loop_step_dev(B, tx, to, tg, X, U, u0, flags=flags, min_margin=mm, ep_flags=fl, ep_steps=ns, **kw)
        if piped:
            for _, _, _, ps in s.parts:
                ps.synchronize()
        torch.cuda.synchronize()
        us.append(u0.cpu().numpy().copy())
    res = dict(x=tx.cpu().numpy(), obst=to.cpu().numpy(), X=X.cpu().numpy(), U=U.cpu().numpy(), u0=np.array(us), mm=mm.cpu().numpy(),
               fl=fl.cpu().numpy(), ns=ns.cpu().numpy())
    if solver is None:
        s.close()
    return res


def _host_driven(mpc_gpu, N, no, B, steps, x0, goal, obst, act, b1, b2, R, path):
    """the same steps through mpc_solve_obst + mpc_plant_step + mpc_shift (and the obstacle motion kernel), set_instance_bounds called at the same step,
    the bookkeeping in numpy over the present obstacles: an instance that has reached its goal idles, nothing of it is touched"""
    import torch
    dev = torch.device("cuda", 0)
    x, ob = x0.copy(), obst.copy()
    alive = np.ones(B, bool)
    mm = np.full(B, np.inf); ns = np.zeros(B, np.int32); fl = np.zeros(B, np.int32)
    us, u_last = [], np.zeros((B, 2))
    off = np.zeros(B, np.int32)
    r_hit = np.full((B, no), 1.2) if R is None else R - (2.4 - 1.2)
    with make(mpc_gpu, N, no, B) as s:
        if R is not None:
            s.set_instance_params(r_safe=R)
        s.set_obstacle_mask(act)
        s.reset_guess(x)
        ar = [float(v) for v in s.cfg.arena]
        for k in range(steps):
            s.set_instance_bounds(**(b1 if k < steps // 2 else b2))
            Xk, Uk = s.get_traj(B)
            if path is not None:
                s.set_reference(path, offset=off)
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
            dist = np.linalg.norm(x[:, None, :2] - ob[:, :, :2], axis=2) - r_hit
            margin = np.where(act, dist, np.inf).min(axis=1)
            mm[alive] = np.minimum(mm, margin)[alive]
            a_ = x[:, 0]; b_ = x[:, 1]
            fl[alive & ((a_ < ar[0]) | (a_ > ar[1]) | (b_ < ar[2]) | (b_ > ar[3]))] |= 2
            fl[alive & (mm <= 0.0)] |= 4
            reached = np.linalg.norm(x[:, :2] - goal, axis=1) <= 0.15
            fl[alive & reached] |= 1
            ns[alive & ~reached] += 1
            alive &= ~reached
            us.append(u_last.copy())
        X, U = s.get_traj(B)
    return dict(x=x, obst=ob, X=X, U=U, u0=np.array(us), mm=mm, ns=ns, fl=fl)


def _body_fused_equals_host(mg, N, no, extras):
    mpc_gpu, _ = mg
    B, steps = 8, 10
    x0, goal, obst, act, b1, b2, R, path = loop_inputs(N, no, B, 740 + N + no, steps, extras)
    assert not np.array_equal(b1["bu_hi"], b2["bu_hi"]) and not act.all() and act.any()
    f = _fused(mpc_gpu, N, no, B, steps, x0, goal, obst, act, b1, b2, R, path)
    h = _host_driven(mpc_gpu, N, no, B, steps, x0, goal, obst, act, b1, b2, R, path)
    for k in ("x", "obst", "X", "U", "u0", "ns"):
        assert np.array_equal(f[k], h[k]), k
    both = np.isfinite(h["mm"])
    assert np.array_equal(np.isfinite(f["mm"]), both)
    assert np.abs(f["mm"][both] - h["mm"][both]).max(initial=0.0) <= 1e-12      # (numpy's norm against the kernel's sqrt of a contracted sum)
    margin_clear = np.abs(h["mm"]) > 1e-9
    assert np.array_equal(f["fl"][margin_clear], h["fl"][margin_clear])


@pytest.mark.parametrize("N,no,extras", [(20, 3, True), (50, 10, False), (20, 15, False)])
def test_fused_loop_equals_host_driven_steps(mg, N, no, extras):
    _on_own_stream(_body_fused_equals_host, mg, N, no, extras)


# ---------------------------------------------------------------------------------------------------------------- 5. pipelined sub-batches
def _body_pipelined(mg):
    mpc_gpu, _ = mg
    N, no, B, steps = 20, 3, 10, 8
    x0, goal, obst, act, b1, b2, R, path = loop_inputs(N, no, B, 1013, steps, True)
    one = _fused(mpc_gpu, N, no, B, steps, x0, goal, obst, act, b1, b2, R, path)
    from mpc_gpu.pipeline import PipelinedMpc
    with PipelinedMpc(N, no, 0.1 * N, max_batch=B, streams=2) as p:
        for _, _, m, _ in p.parts:
            m.set_instance_scheduling(False)
        assert not p.kernel_name().endswith(", true>")                  # (nothing set yet)
        two = _fused(mpc_gpu, N, no, B, steps, x0, goal, obst, act, b1, b2, R, path, solver=p)
        assert p.kernel_name().endswith(LEVEL4)
        p.set_instance_bounds_dev(None)
        assert p.kernel_name().endswith(", true, true, true>") and not p.kernel_name().endswith(LEVEL4)      # (the mask, the radii and the reference stay)
        p.set_instance_bounds(**b1)                                     # the host form, cut per part
        assert p.kernel_name().endswith(LEVEL4)
    for k in one:
        assert np.array_equal(one[k], two[k]), k


def test_pipelined_sub_batches_equal_one_handle(mg):
    _on_own_stream(_body_pipelined, mg)


# ---------------------------------------------------------------------------------------------------------------- 6. refusals and switching off
def test_refusals_and_switching_off(mg):
    import torch
    mpc_gpu, _ = mg
    L = mpc_gpu._lib
    N, no, B = 20, 3, 4
    x0, goal, obst = random_batch(B, no, seed=3)
    x0[:, 3:] = 0.0
    tight = dict(bu_lo=np.tile([-1.5, -2.0], (B, 1)), bu_hi=np.tile([2.0, 1.5], (B, 1)), bx_lo=np.tile([-7.0, -7.0, -0.9, -1.0], (B, 1)))
    for setup in (lambda s: s.set_matrix_cores(True), lambda s: s.set_row_parallel(False), lambda s: s.set_block_riccati(True),
                  lambda s: s.set_lanes_per_instance(32)):
        with mpc_gpu.BatchedMpc(N, no, 2.0, max_batch=B) as s:
            setup(s)
            s.set_instance_bounds(**tight)
            with pytest.raises(mpc_gpu.MpcError, match="instance bounds") as e:
                s.solve(x0, obst, goal)
            assert f"libmpcgpu error {L.MPC_ERR_ARG}" in str(e.value)
            with pytest.raises(mpc_gpu.MpcError, match="instance bounds"):
                s.kernel_name(B)
    with pytest.raises(mpc_gpu.MpcError, match="N <= 31"):              # more than 10 obstacles beyond two lanes per stage: refused as before, at creation
        mpc_gpu.BatchedMpc(40, 15, 4.0, max_batch=B)
    with mpc_gpu.BatchedMpc(N, no, 2.0, max_batch=B) as s, mpc_gpu.BatchedMpc(N, no, 2.0, max_batch=B) as fresh:
        s.set_instance_scheduling(False); fresh.set_instance_scheduling(False)
        h, lib = s._h, L.lib()
        lo2, hi2, lo4, hi4 = -np.ones((B + 1, 2)), np.ones((B + 1, 2)), -np.ones((B + 1, 4)), np.ones((B + 1, 4))
        p = lambda a: None if a is None else a.ctypes.data
        call = lambda n, bx_lo=None, bx_hi=None, bu_lo=None, bu_hi=None: lib.mpc_set_instance_bounds(h, n, p(bx_lo), p(bx_hi), p(bu_lo), p(bu_hi))

        def put(a, v, at=(B - 1, 1)):
            a = a.copy(); a[at] = v
            return a
        refused = [(0, dict(bu_lo=lo2), b"batch"), (B + 1, dict(bu_lo=lo2), b"batch"),
                   (B, dict(bu_lo=put(lo2, np.nan)), b"bu_lo"), (B, dict(bx_hi=put(hi4, np.inf)), b"bx_hi"), (B, dict(bx_lo=put(lo4, -np.inf)), b"bx_lo"),
                   (B, dict(bu_lo=lo2, bu_hi=put(hi2, -1.0)), b"bu_hi"),                 # lo == hi
                   (B, dict(bx_lo=lo4, bx_hi=put(hi4, -2.0)), b"bx_lo"),                 # lo > hi
                   (B, dict(bu_hi=put(hi2, -8.0)), b"bu_hi"),                            # one side given: against the handle's bu_lo = -8 (equal)
                   (B, dict(bx_lo=put(lo4, 10.5, at=(0, 3))), b"bx_lo")]                 # ... and above the handle's bx_hi = 10
        for n, bad, word in refused:
            assert call(n, **bad) == L.MPC_ERR_ARG, (n, word)
            assert word in lib.mpc_last_error(), (word, lib.mpc_last_error())           # the message names the field
            assert s.kernel_name(B) == fresh.kernel_name(B)                              # nothing refused switched the feature on
        assert call(B, bu_lo=lo2) == L.MPC_OK and s.kernel_name(B).endswith(LEVEL4)
        # fewer instances than the solve
        s.set_instance_bounds(**{k: v[:2] for k, v in tight.items()})
        with pytest.raises(mpc_gpu.MpcError, match="fewer instances"):
            s.solve(x0, obst, goal)
        # on, then off (both forms): the parent's kernel and a fresh handle's results, bit for bit
        want = run(fresh, x0, obst, goal, 2)
        s.set_instance_bounds(**tight)
        assert s.kernel_name(B).endswith(LEVEL4) and s.kernel_name(B) != fresh.kernel_name(B)
        changed = run(s, x0, obst, goal, 2)
        s.set_instance_bounds()
        assert s.kernel_name(B) == fresh.kernel_name(B)
        assert_same(run(s, x0, obst, goal, 2), want)
        assert not np.array_equal(changed[0][1], want[0][1])            # (and the bounds did reach the solve while they were on)
        table = torch.tensor(mpc_gpu.pack_instance_bounds(s.cfg, B, **tight), device="cuda")
        s.set_instance_bounds_dev(table)
        assert s.kernel_name(B).endswith(LEVEL4)
        assert_same(run(s, x0, obst, goal, 2), changed)                 # the device form is the host form
        s.set_instance_bounds_dev(None)
        assert s.kernel_name(B) == fresh.kernel_name(B)
        assert_same(run(s, x0, obst, goal, 2), want)
        # the bounds survive a mask and instance parameters coming and going
        s.set_instance_bounds(**tight)
        some = np.array([[1, 0, 1], [0, 1, 0], [1, 1, 1], [0, 0, 0]], bool)
        s.set_obstacle_mask(some)
        assert s.kernel_name(B).endswith(LEVEL4)
        masked = run(s, x0, obst, goal, 2)
        assert not np.array_equal(masked[0][1], changed[0][1])
        s.set_obstacle_mask(None)
        assert_same(run(s, x0, obst, goal, 2), changed)
        s.set_instance_params(r_safe=np.full(B, 1.7))
        assert s.kernel_name(B).endswith(LEVEL4)
        s.set_instance_params()
        assert_same(run(s, x0, obst, goal, 2), changed)
        # ... and leave a masked handle as it was: level 3 again, the results of a handle that never had bounds
        s.set_obstacle_mask(some); fresh.set_obstacle_mask(some)
        s.set_instance_bounds()
        assert s.kernel_name(B) == fresh.kernel_name(B) and s.kernel_name(B).endswith(", true, true, true>")
        assert_same(run(s, x0, obst, goal, 2), run(fresh, x0, obst, goal, 2))


# ---------------------------------------------------------------------------------------------------------------- 7. run_episodes
def _steps(mpc_gpu, s, B, N, x0, goal, obst, steps):
    import torch
    L = mpc_gpu._lib
    dev = torch.device("cuda", 0)
    tt = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)
    tx, to, tg = tt(x0), tt(obst), tt(goal)
    X = torch.zeros((B, N + 1, 5), dtype=torch.float64, device=dev); U = torch.zeros((B, N, 2), dtype=torch.float64, device=dev)
    mm = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
    fl = torch.zeros(B, dtype=torch.int32, device=dev); ns = torch.zeros(B, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    s.reset_guess_dev(B, tx, X, U, stream=st)
    for k in range(steps):
        s.closed_loop_step_dev(B, tx, to, tg, X, U, flags=L.STEP_SHIFT | L.STEP_PLANT | L.STEP_OBSTACLES | L.STEP_METRICS,
                               min_margin=mm, ep_flags=fl, ep_steps=ns, stream=st)
    torch.cuda.synchronize()
    return dict(x=tx.cpu().numpy(), mm=mm.cpu().numpy())


def _body_episodes(mg):
    mpc_gpu, _ = mg
    from mpc_gpu.episodes import run_episodes
    B, no, N, steps = 8, 3, 20, 5
    x0, goal, obst = random_batch(B, no, seed=12)
    x0[:, 3:] = 0.0
    kw = dict(N=N, Tf=2.0, max_iter=steps, random_move=False, bug_compat_alias=False, init_guess_when_error=False, n_obst=no)
    base = run_episodes(x0, goal, obst, **kw)
    same = run_episodes(x0, goal, obst, bounds={k: np.tile(v, (B, 1)) for k, v in DEFAULTS.items()}, **kw)
    tight = dict(bu_lo=np.array([-1.0, -1.5]), bu_hi=np.tile([1.5, 1.0], (B, 1)))      # one row for all, and rows of their own
    got = run_episodes(x0, goal, obst, bounds=tight, **kw)
    assert np.array_equal(same["table"], base["table"]) and np.array_equal(same["x_last"], base["x_last"])
    assert not np.array_equal(got["x_last"], base["x_last"])
    # the step API on the same inputs
    with mpc_gpu.BatchedMpc(N, no, 2.0, max_batch=B) as s:
        s.set_instance_bounds(**tight)
        r = _steps(mpc_gpu, s, B, N, x0, goal, obst, steps)
    assert np.array_equal(got["x_last"], r["x"]) and np.array_equal(got["table"][:, 2], r["mm"])


def test_run_episodes_passes_the_bounds_through(mg):
    _on_own_stream(_body_episodes, mg)
