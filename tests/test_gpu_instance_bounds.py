"""Per-instance box bounds (mpc_set_instance_bounds, BatchedMpc.set_instance_bounds, PipelinedMpc.set_instance_bounds_dev) on the GPU: uniform bounds are
the configured handle bit for bit on all eleven instantiations, a mixed batch is its groups bit for bit, mixed bounds are judged against the oracle
group by group, the fused loop equals host-driven steps with the table rewritten on the device, pipelined sub-batches equal one handle, the refusals
and switching off, and run_episodes."""
import numpy as np
import pytest

from feature_loop import (FeatureStack, assert_fused_equals_host, assert_same, fused_loop, host_driven_loop, level_of, make, mg, on_own_stream,
                          resident_steps, run, smooth_path)
from helpers import allowed_adjudications, judge_against_oracle, oracle_P, oracle_reference, random_batch
from instance_bounds_cases import DEFAULTS, as_cfg, draw_bounds, per_instance
from obstacle_mask_cases import draw_masks

pytestmark = pytest.mark.gpu

# split x3 / split x2 on 3, 5, 10 rows; one instance per wavefront on 3, 5, 10 rows; the multi-wavefront kernel on 20 and 32 rows: the eleven instantiations
ALL_SIZES = [(20, 3), (30, 3), (20, 5), (30, 5), (20, 10), (30, 10), (50, 3), (50, 5), (50, 10), (20, 15), (20, 25)]
LEVEL4 = ", true, true, true, true>"
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
    on_own_stream(_body_uniform, mg, N, no)


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
    on_own_stream(_body_groups, mg, N, no)


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
    on_own_stream(_body_oracle, mg, N, no, B, seed, bx_terminal)


# ---------------------------------------------------------------------------------------------------------------- 4. fused loop = host-driven steps
def loop_inputs(N, no, B, seed, steps, extras):
    rng = np.random.default_rng(seed)
    x0, goal, obst = random_batch(B, no, seed=seed)
    x0[:, 3:] = 0.0
    act = draw_masks(rng, B, no)
    b1, b2 = per_instance(*draw_bounds(rng, B)), per_instance(*draw_bounds(rng, B))
    R = rng.uniform(1.6, 3.0, (B, no)) if extras else None
    path = smooth_path(rng, B, steps + N + 1) if extras else None
    return FeatureStack(r_safe=R, mask=act, bounds=(b1, b2), path=path), x0, goal, obst


def _body_fused_equals_host(mg, N, no, extras):
    mpc_gpu, _ = mg
    B, steps = 8, 10
    stack, x0, goal, obst = loop_inputs(N, no, B, 740 + N + no, steps, extras)
    (b1, b2), act = stack.bounds, stack.mask
    assert not np.array_equal(b1["bu_hi"], b2["bu_hi"]) and not act.all() and act.any()
    f = fused_loop(mpc_gpu, N, no, B, steps, x0, goal, obst, stack)
    h = host_driven_loop(mpc_gpu, N, no, B, steps, x0, goal, obst, stack)
    assert_fused_equals_host(f, h)


@pytest.mark.parametrize("N,no,extras", [(20, 3, True), (50, 10, False), (20, 15, False)])
def test_fused_loop_equals_host_driven_steps(mg, N, no, extras):
    on_own_stream(_body_fused_equals_host, mg, N, no, extras)


# ---------------------------------------------------------------------------------------------------------------- 5. pipelined sub-batches
def _body_pipelined(mg):
    mpc_gpu, _ = mg
    N, no, B, steps = 20, 3, 10, 8
    stack, x0, goal, obst = loop_inputs(N, no, B, 1013, steps, True)
    one = fused_loop(mpc_gpu, N, no, B, steps, x0, goal, obst, stack)
    from mpc_gpu.pipeline import PipelinedMpc
    with PipelinedMpc(N, no, 0.1 * N, max_batch=B, streams=2) as p:
        for _, _, m, _ in p.parts:
            m.set_instance_scheduling(False)
        assert not p.kernel_name().endswith(", true>")                  # (nothing set yet)
        two = fused_loop(mpc_gpu, N, no, B, steps, x0, goal, obst, stack, solver=p)
        assert p.kernel_name().endswith(LEVEL4)
        p.set_instance_bounds_dev(None)
        assert p.kernel_name().endswith(", true, true, true>") and not p.kernel_name().endswith(LEVEL4)      # (the mask, the radii and the reference stay)
        p.set_instance_bounds(**stack.bounds[0])                        # the host form, cut per part
        assert p.kernel_name().endswith(LEVEL4)
    for k in one:
        assert np.array_equal(one[k], two[k]), k


def test_pipelined_sub_batches_equal_one_handle(mg):
    on_own_stream(_body_pipelined, mg)


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
        r = resident_steps(mpc_gpu, s, B, N, x0, goal, obst, steps)
    assert np.array_equal(got["x_last"], r["x"][-1]) and np.array_equal(got["table"][:, 2], r["mm"])


def test_run_episodes_passes_the_bounds_through(mg):
    on_own_stream(_body_episodes, mg)
