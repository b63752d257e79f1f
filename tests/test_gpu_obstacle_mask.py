"""Per-instance obstacle masks (mpc_set_obstacle_mask, BatchedMpc.set_obstacle_mask, PipelinedMpc.set_obstacle_mask_dev) on the GPU: a full mask is the
per-instance-parameter path, a prefix mask is the smaller handle bit for bit, what absent entries hold is ignored, arbitrary masks are judged against
the oracle group by group, the mask reaches constraint, cost and metrics, the fused loop equals host-driven steps with the words rewritten on the
device, pipelined sub-batches equal one handle, the refusals, and run_episodes."""
import numpy as np
import pytest

from feature_loop import (FeatureStack, assert_fused_equals_host, assert_same, cfg_values, fused_loop, host_driven_loop, make, mg, on_own_stream,
                          resident_steps, run, smooth_path)
from helpers import allowed_adjudications, judge_against_oracle, oracle_P, oracle_reference, random_batch
from instance_params_qp import cost as np_cost
from obstacle_mask_cases import active_columns, draw_masks, groups, poison

pytestmark = pytest.mark.gpu

SIZES = [(20, 3), (20, 5), (30, 10), (20, 15), (50, 10)]      # split x3, split x3 on five rows, split x2 on ten rows, the multi-wavefront kernel, one instance per wavefront
PREFIX = [(20, 5, 4), (30, 10, 7), (20, 15, 12), (50, 10, 7)]


# ---------------------------------------------------------------------------------------------------------------- 1. a full mask is the IPAR path
def _body_full(mg, N, no):
    mpc_gpu, orc = mg
    B = 8
    x0, goal, obst = random_batch(B, no, seed=11 * N + no + B)
    cfg = orc.config(N, no, 0.1 * N)
    with make(mpc_gpu, N, no, B) as m, make(mpc_gpu, N, no, B) as r:
        W, We, rs = cfg_values(r)
        r.set_instance_params(W=np.tile(W, (B, 1)), We=np.tile(We, (B, 1)), r_safe=np.full((B, no), rs))
        m.set_obstacle_mask(np.ones((B, no), bool))
        name = m.kernel_name(B)
        print(N, no, "mask:", name, "| instance parameters:", r.kernel_name(B))
        assert name.endswith(", true, true, true>"), name
        assert name.split("<")[0] == r.kernel_name(B).split("<")[0]                      # the same family
        assert_same(run(r, x0, obst, goal), run(m, x0, obst, goal), cost_rtol=1e-13)                      # look-ahead in the kernel
        P = oracle_P(orc, cfg, obst)
        assert_same(run(r, x0, P, goal, 2), run(m, x0, P, goal, 2), cost_rtol=1e-13)                      # explicit P
        m.set_instance_params(W=np.tile(W, (B, 1)))                                      # the mask on top of instance parameters: still the same
        assert m.kernel_name(B) == name
        assert_same(run(r, x0, obst, goal, 2), run(m, x0, obst, goal, 2), cost_rtol=1e-13)


@pytest.mark.parametrize("N,no", SIZES)
def test_full_mask_is_the_instance_parameter_path(mg, N, no):
    on_own_stream(_body_full, mg, N, no)


# ---------------------------------------------------------------------------------------------------------------- 2. a prefix mask is the smaller handle
def _body_prefix(mg, N, no, k):
    mpc_gpu, orc = mg
    B = 8
    x0, goal, obst = random_batch(B, no, seed=13 * N + no + k)
    act = np.zeros((B, no), bool); act[:, :k] = True
    with make(mpc_gpu, N, no, B) as big:
        thr0 = float(big.cfg.thr0)
        with make(mpc_gpu, N, k, B, thr0=thr0) as small:
            assert float(small.cfg.thr0) == thr0
            big.set_obstacle_mask(act)
            small.set_obstacle_mask(np.ones((B, k), bool))
            assert big.kernel_name(B) == small.kernel_name(B), (big.kernel_name(B), small.kernel_name(B))      # same row capacity, same mapping
            assert_same(run(big, x0, obst, goal), run(small, x0, obst[:, :k].copy(), goal))
            P = oracle_P(orc, orc.config(N, no, 0.1 * N), obst)
            assert_same(run(big, x0, P, goal, 2), run(small, x0, np.ascontiguousarray(P[:, :, :k]), goal, 2))


@pytest.mark.parametrize("N,no,k", PREFIX)
def test_prefix_mask_is_the_smaller_handle(mg, N, no, k):
    on_own_stream(_body_prefix, mg, N, no, k)


# ---------------------------------------------------------------------------------------------------------------- 3. absent entries are ignored
def _on_the_robot(arr, act, x0):
    out = np.array(arr, copy=True)
    B = out.shape[0]
    for b in range(B):
        for j in np.nonzero(~act[b])[0]:
            if out.ndim == 3:
                out[b, j] = (x0[b, 0], x0[b, 1], 0.0, 0.0)
            else:
                out[b, :, j] = x0[b, :2]
    return out


def _body_absent(mg, N, no):
    mpc_gpu, orc = mg
    B = 12
    rng = np.random.default_rng(700 + N + no)
    x0, goal, obst = random_batch(B, no, seed=19 * N + no)
    act = draw_masks(rng, B, no)
    P = oracle_P(orc, orc.config(N, no, 0.1 * N), obst)
    with make(mpc_gpu, N, no, B) as s:
        s.set_obstacle_mask(act)
        fin, fin_P = run(s, x0, obst, goal), run(s, x0, P, goal, 2)
        for what, o_v, P_v in (("nan", poison(obst, act, np.nan), poison(P, act, np.nan)), ("inf", poison(obst, act, np.inf), poison(P, act, np.inf)),
                               ("robot", _on_the_robot(obst, act, x0), _on_the_robot(P, act, x0))):
            got, got_P = run(s, x0, o_v, goal), run(s, x0, P_v, goal, 2)
            assert_same(fin, got)
            assert_same(fin_P, got_P)
            for r in got + got_P:
                assert all(np.isfinite(v).all() for v in r[:4]), what
    print(N, no, "status 4 of the finite variant:", int((fin[0][4] == 4).sum()), "of", B)


@pytest.mark.parametrize("N,no", SIZES)
def test_absent_entries_are_ignored(mg, N, no):
    on_own_stream(_body_absent, mg, N, no)


# ---------------------------------------------------------------------------------------------------------------- 4. arbitrary masks against the oracle
# (N, n_obst, B, seed of random_batch): chosen on the CPU before the first GPU run -- the oracle alone returns status 0 for every instance with at least
# one obstacle present (the counts are in DESIGN.md section 4d)
ORACLE_CASES = [(20, 3, 16, 31), (20, 5, 16, 32), (30, 10, 16, 36), (20, 15, 16, 34), (50, 10, 16, 35)]


def oracle_inputs(N, no, B, seed):
    rng = np.random.default_rng(900 + N + no)
    x0, goal, obst = random_batch(B, no, seed=seed)
    x0[:, 3:] = 0.0
    return x0, goal, obst, draw_masks(rng, B, no)


def _body_oracle(mg, N, no, B, seed):
    mpc_gpu, orc = mg
    x0, goal, obst, act = oracle_inputs(N, no, B, seed)
    assert sorted(set(act.sum(axis=1))) == list(range(min(no, B - 1) + 1))
    cfg = orc.config(N, no, 0.1 * N)
    P = oracle_P(orc, cfg, obst)
    with make(mpc_gpu, N, no, B) as s:
        thr0 = float(s.cfg.thr0)
        s.reset_guess(x0)
        X0, U0 = s.get_traj(B)
        s.set_obstacle_mask(act)
        g = s.solve(x0, poison(P, act, np.nan), goal)
        Xg, Ug = s.get_traj(B)
    judged = 0
    for key, idx in groups(act).items():
        idx = np.array(idx); k = int(sum(key))
        gb = {name: v[idx] for name, v in g.items()}
        if k == 0:      # the oracle has no zero-obstacle form: an unmasked handle whose slack schedule is zero everywhere has no obstacle rows either
            with make(mpc_gpu, N, no, len(idx)) as z:
                z.set_slack_schedule(np.zeros((len(idx), N + 1)))
                z.reset_guess(x0[idx])
                o = z.solve(x0[idx], P[idx], goal[idx])
                Xz, Uz = z.get_traj(len(idx))
            assert np.array_equal(o["status"], gb["status"])
            ok = o["status"] == 0
            print(f"N {N} no {no}: count 0, {int(ok.sum())} of {len(idx)} converged, |dX| {np.abs(Xz - Xg[idx]).max():.2e} |dU| {np.abs(Uz - Ug[idx]).max():.2e}")
            assert np.abs(Xz - Xg[idx])[ok].max(initial=0.0) <= 1e-6 and np.abs(Uz - Ug[idx])[ok].max(initial=0.0) <= 8e-6
            continue
        cfg_k = orc.config(N, k, 0.1 * N, thr0=thr0)
        Pk = np.stack([active_columns(P[b], act[b]) for b in idx])
        o = oracle_reference(orc, cfg_k, x0[idx], Pk, goal[idx], X0[idx], U0[idx])
        n = judge_against_oracle(orc, cfg_k, x0[idx], Pk, goal[idx], X0[idx], U0[idx], gb, Xg[idx], Ug[idx], o)
        print(f"N {N} no {no}: mask {key} ({len(idx)} instances): {n}")
        judged += n["judged_by_qp"]
    assert judged <= allowed_adjudications(cfg, B), judged      # the project's bound holds over the batch, not per group


@pytest.mark.parametrize("N,no,B,seed", ORACLE_CASES)
def test_arbitrary_masks_against_the_oracle(mg, N, no, B, seed):
    on_own_stream(_body_oracle, mg, N, no, B, seed)


# ---------------------------------------------------------------------------------------------------------------- 5. the mask matters
def _body_matters(mg):
    mpc_gpu, orc = mg
    L = mpc_gpu._lib
    N, no, B, steps = 20, 2, 8, 12
    rng = np.random.default_rng(77)
    x0 = np.zeros((B, 5)); x0[:, 0] = -3.0; x0[:, 1] = rng.uniform(-0.2, 0.2, B)
    goal = np.zeros((B, 2)); goal[:, 0] = 5.0
    obst = np.zeros((B, no, 4))
    obst[:, 0, 0] = -1.0; obst[:, 0, 1] = 0.3; obst[:, 0, 2:] = (0.2, 0.1)      # obstacle 0: on the robot's path, 2 m ahead -- inside the safety radius 2.4 from the start
    obst[:, 1, 0] = 4.0; obst[:, 1, 1] = 5.5; obst[:, 1, 2:] = (-0.3, 0.2)      # obstacle 1: far off
    noise = rng.standard_normal((steps, B, no, 2))
    on = np.ones((B, no), bool); off = on.copy(); off[:, 0] = False
    with make(mpc_gpu, N, no, B) as s, make(mpc_gpu, N, no, B) as plain:
        s.set_obstacle_mask(on); a = resident_steps(mpc_gpu, s, B, N, x0, goal, obst, steps, noise)
        s.set_obstacle_mask(off); b = resident_steps(mpc_gpu, s, B, N, x0, goal, obst, steps, noise)
        c = resident_steps(mpc_gpu, s, B, N, x0, goal, obst, steps, noise, L.STEP_MARGIN_ALL)
        u = resident_steps(mpc_gpu, plain, B, N, x0, goal, obst, steps, noise)
        # the reported cost of the first solve, term for term: with the obstacle and without it
        s.reset_guess(x0); ob = s.solve(x0, obst, goal); Xb, Ub = s.get_traj(B)
        s.set_obstacle_mask(on); s.reset_guess(x0); oa = s.solve(x0, obst, goal); Xa, Ua = s.get_traj(B)
    cfg2, cfg1 = orc.config(N, 2, 0.1 * N), orc.config(N, 1, 0.1 * N)
    W0 = np.array([cfg2.W[k] for k in range(6)]); We0 = np.array([cfg2.We[k] for k in range(4)])
    P = oracle_P(orc, cfg2, obst)
    for i in range(B):
        Ja = np_cost(cfg2, x0[i], goal[i], Xa[i], Ua[i], P[i], W0, We0, np.full(2, float(cfg2.r_safe)))
        Jb = np_cost(cfg1, x0[i], goal[i], Xb[i], Ub[i], P[i][:, 1:], W0, We0, np.full(1, float(cfg2.r_safe)))
        Jb_with = np_cost(cfg2, x0[i], goal[i], Xb[i], Ub[i], P[i], W0, We0, np.full(2, float(cfg2.r_safe)))
        assert abs(oa["cost"][i] - Ja) <= 1e-10 * max(1.0, abs(Ja)) and abs(ob["cost"][i] - Jb) <= 1e-10 * max(1.0, abs(Jb)), (i, oa["cost"][i], Ja, ob["cost"][i], Jb)
        assert Jb_with > Jb + 1.0                                    # (the penalty the masked cost lacks is there to be lacked)
    assert np.abs(a["u0"][0] - b["u0"][0]).max() > 1e-3              # the obstacle reaches the solve when it is present
    for k in ("u0", "cost", "x", "X", "U"):
        assert np.array_equal(b[k], c[k]), k                         # MARGIN_ALL: bookkeeping only
    for r in (a, b, c):
        assert np.array_equal(r["obst"], u["obst"])                  # every obstacle moved and drew its noise, present or not
    assert np.array_equal(a["x"], u["x"]) and np.array_equal(a["mm"], u["mm"]) and np.array_equal(a["fl"], u["fl"])
    d = lambda r, cols: (np.linalg.norm(r["x"][:, :, None, :2] - r["obst"][:, :, cols, :2], axis=3) - 1.2).min(axis=(0, 2))
    print("min margin: on", a["mm"], "off", b["mm"], "off + MARGIN_ALL", c["mm"])
    assert np.abs(b["mm"] - d(b, [1])).max() <= 1e-12                # masked off: the margin ignores obstacle 0
    assert np.abs(c["mm"] - d(c, [0, 1])).max() <= 1e-12             # MARGIN_ALL: the bookkeeping of an unmasked handle on this trajectory
    assert (b["mm"] > 1.0).all() and (c["mm"] < 0.0).all()           # (the blind robot drives through obstacle 0)
    assert ((b["fl"] & 4) == 0).all() and ((c["fl"] & 4) == 4).all()
    assert (a["mm"] > c["mm"] + 0.5).all()                           # (and the robot that sees it keeps away)


def test_mask_reaches_constraint_cost_and_metrics(mg):
    on_own_stream(_body_matters, mg)


# ---------------------------------------------------------------------------------------------------------------- 6. fused loop = host-driven steps
def loop_inputs(N, no, B, seed, steps, extras):
    rng = np.random.default_rng(seed)
    x0, goal, obst = random_batch(B, no, seed=seed)
    x0[:, 3:] = 0.0
    act1, act2 = draw_masks(rng, B, no), draw_masks(rng, B, no)
    R = rng.uniform(1.6, 3.0, (B, no)) if extras else None
    path = smooth_path(rng, B, steps + N + 1) if extras else None
    return FeatureStack(r_safe=R, mask=(act1, act2), path=path), x0, goal, obst


def _body_fused_equals_host(mg, N, no, extras):
    mpc_gpu, _ = mg
    B, steps = 8, 10
    stack, x0, goal, obst = loop_inputs(N, no, B, 640 + N + no, steps, extras)
    assert not np.array_equal(*stack.mask)
    f = fused_loop(mpc_gpu, N, no, B, steps, x0, goal, obst, stack)
    h = host_driven_loop(mpc_gpu, N, no, B, steps, x0, goal, obst, stack)
    assert_fused_equals_host(f, h)


@pytest.mark.parametrize("N,no,extras", [(20, 3, True), (30, 10, False), (20, 15, False), (50, 10, False)])
def test_fused_loop_equals_host_driven_steps(mg, N, no, extras):
    on_own_stream(_body_fused_equals_host, mg, N, no, extras)


# ---------------------------------------------------------------------------------------------------------------- 7. pipelined sub-batches
def _body_pipelined(mg):
    mpc_gpu, _ = mg
    N, no, B, steps = 20, 3, 10, 8
    stack, x0, goal, obst = loop_inputs(N, no, B, 913, steps, True)
    one = fused_loop(mpc_gpu, N, no, B, steps, x0, goal, obst, stack)
    from mpc_gpu.pipeline import PipelinedMpc
    with PipelinedMpc(N, no, 0.1 * N, max_batch=B, streams=2) as p:
        for _, _, m, _ in p.parts:
            m.set_instance_scheduling(False)
        assert not p.kernel_name().endswith(", true, true, true>")      # (nothing set yet)
        two = fused_loop(mpc_gpu, N, no, B, steps, x0, goal, obst, stack, solver=p)
        assert p.kernel_name().endswith(", true, true, true>")
        p.set_obstacle_mask_dev(None)
        assert p.kernel_name().endswith(", true, true>") and not p.kernel_name().endswith(", true, true, true>")      # (the radii and the reference stay)
    for k in one:
        assert np.array_equal(one[k], two[k]), k


def test_pipelined_sub_batches_equal_one_handle(mg):
    on_own_stream(_body_pipelined, mg)


# ---------------------------------------------------------------------------------------------------------------- 8. refusals and switching off
def test_refusals_and_switching_off(mg):
    mpc_gpu, _ = mg
    L = mpc_gpu._lib
    N, no, B = 20, 3, 4
    x0, goal, obst = random_batch(B, no, seed=3)
    some = np.array([[1, 0, 1], [0, 1, 0], [1, 1, 1], [0, 0, 0]], bool)
    for setup in (lambda s: s.set_matrix_cores(True), lambda s: s.set_row_parallel(False), lambda s: s.set_block_riccati(True),
                  lambda s: s.set_lanes_per_instance(32)):
        with mpc_gpu.BatchedMpc(N, no, 2.0, max_batch=B) as s:
            setup(s)
            s.set_obstacle_mask(some)
            with pytest.raises(mpc_gpu.MpcError, match="obstacle mask") as e:
                s.solve(x0, obst, goal)
            assert f"libmpcgpu error {L.MPC_ERR_ARG}" in str(e.value)
            with pytest.raises(mpc_gpu.MpcError, match="obstacle mask"):
                s.kernel_name(B)
    with mpc_gpu.BatchedMpc(N, no, 2.0, max_batch=B) as s, mpc_gpu.BatchedMpc(N, no, 2.0, max_batch=B) as fresh:
        s.set_instance_scheduling(False); fresh.set_instance_scheduling(False)
        h, lib = s._h, L.lib()
        w = lambda *v: np.array(v, np.uint32)
        assert lib.mpc_set_obstacle_mask(h, 0, w(1).ctypes.data) == L.MPC_ERR_ARG
        assert lib.mpc_set_obstacle_mask(h, B + 1, w(1, 1, 1, 1, 1).ctypes.data) == L.MPC_ERR_ARG
        for bad in (w(7, 8, 7, 7), w(7, 7, 7, 0x80000000), w(15, 0, 0, 0)):
            assert lib.mpc_set_obstacle_mask(h, B, bad.ctypes.data) == L.MPC_ERR_ARG
            assert b"n_obst" in lib.mpc_last_error()
        assert s.kernel_name(B) == fresh.kernel_name(B)                  # nothing refused above switched the feature on
        assert lib.mpc_set_obstacle_mask(h, B, w(7, 0, 5, 2).ctypes.data) == L.MPC_OK      # an empty word is a word
        # fewer instances than the solve
        s.set_obstacle_mask(some[:2])
        with pytest.raises(mpc_gpu.MpcError, match="fewer instances"):
            s.solve(x0, obst, goal)
        # on, then off: the parent's kernel and a fresh handle's results, bit for bit
        s.set_obstacle_mask(some)
        assert s.kernel_name(B).endswith(", true, true, true>") and s.kernel_name(B) != fresh.kernel_name(B)
        changed = run(s, x0, obst, goal, 2)
        s.set_obstacle_mask(None)
        assert s.kernel_name(B) == fresh.kernel_name(B)
        back, want = run(s, x0, obst, goal, 2), run(fresh, x0, obst, goal, 2)
        assert_same(back, want)
        assert not np.array_equal(changed[0][0], want[0][0])               # (and the words did reach the solve while they were on)
        # the mask survives instance parameters coming and going
        s.set_obstacle_mask(some)
        with_mask = run(s, x0, obst, goal, 2)
        assert_same(with_mask, changed)
        s.set_instance_params(r_safe=np.full(B, 1.7)); s.set_instance_params()
        assert_same(run(s, x0, obst, goal, 2), changed)


# ---------------------------------------------------------------------------------------------------------------- 9. run_episodes
def _body_episodes(mg):
    mpc_gpu, _ = mg
    from mpc_gpu.episodes import run_episodes
    L = mpc_gpu._lib
    B, no, N, steps = 8, 3, 20, 5
    rng = np.random.default_rng(21)
    x0, goal, obst = random_batch(B, no, seed=12)
    x0[:, 3:] = 0.0
    act = draw_masks(rng, B, no)
    kw = dict(N=N, Tf=2.0, max_iter=steps, random_move=False, bug_compat_alias=False, init_guess_when_error=False, n_obst=no)
    base = run_episodes(x0, goal, obst, **kw)
    got = run_episodes(x0, goal, obst, active=act, **kw)
    allm = run_episodes(x0, goal, obst, active=act, margin_all=True, **kw)
    full = run_episodes(x0, goal, obst, active=np.ones((B, no), bool), **kw)
    assert np.array_equal(full["table"], base["table"]) and np.array_equal(full["x_last"], base["x_last"])
    assert not np.array_equal(got["x_last"], base["x_last"])
    assert np.array_equal(got["x_last"], allm["x_last"])
    # the step API on the same inputs
    with mpc_gpu.BatchedMpc(N, no, 2.0, max_batch=B) as s:
        s.set_obstacle_mask(act)
        r = resident_steps(mpc_gpu, s, B, N, x0, goal, obst, steps, np.zeros((steps, B, no, 2)))
        ra = resident_steps(mpc_gpu, s, B, N, x0, goal, obst, steps, np.zeros((steps, B, no, 2)), L.STEP_MARGIN_ALL)
    assert np.array_equal(got["x_last"], r["x"][-1]) and np.array_equal(got["table"][:, 2], r["mm"])
    assert np.array_equal(allm["table"][:, 2], ra["mm"])
    assert np.isinf(got["table"][act.sum(axis=1) == 0, 2]).all()         # no obstacle, no margin


def test_run_episodes_passes_the_mask_through(mg):
    on_own_stream(_body_episodes, mg)
