"""Shared cases of the sweep-trace tests (test_sweep_trace_host.py, test_gpu_sweep_trace.py).

`batch_trace` is the yardstick of the GPU tests: the path that exists without the feature.  It runs run_episodes' own loop on ONE batch that holds every
seed -- the scenario by name, noise_state / noise_draw_dev, closed_loop_step_dev with run_episodes' step flags and a u0 buffer, compaction off -- and clones
x0, obst, X, u0, status and iters behind each step.  Its first assertion holds it to the committed path: simX / obst_traj / pred equal
run_episodes(..., record=True)'s bit for bit.  Computed once per (mapping, seeds, options), shared, read-only."""
import numpy as np

import sweep_cases as sc

TRACE_FIELDS = ["seed_row", "slot_state", "len", "x", "obst", "u", "status", "iters", "pred"]
NEW = ("mpc_episode_trace_set_dev", "mpc_episode_trace_dev")

# bytes of a trace by hand: 3 seeds, 10 control steps, N 20, 5 obstacles.  Per seed: x 11 * 5 * 8 = 440, obst 11 * 5 * 4 * 8 = 1760, u 10 * 2 * 8 = 160,
# status + iters 2 * 10 * 4 = 80, len 4 -> 2444; pred 10 * 21 * 5 * 8 = 8400 -> 10844
BYTES_CASE = dict(rows=3, max_iter=10, N=20, n_obst=5, without_pred=3 * 2444, with_pred=3 * 10844)


def synthetic_result(L=(4, 7), N=6, n_obst=2, seed=5):
    """a run_seed_sweep result with a hand-made trace of seed indices 1 and 3 out of 4 (lengths L): random numbers, the right shapes"""
    rng = np.random.default_rng(seed)
    table = np.zeros((4, 6)); x_last = rng.normal(size=(4, 5))
    trace = {}
    for k, n in zip((1, 3), L):
        table[k, 4], table[k, 1] = n - 1, 1                    # reached the goal in its n-th control step
        trace[k] = dict(simX=rng.normal(size=(n + 1, 5)), obst_traj=rng.normal(size=(n + 1, n_obst, 4)), u=rng.normal(size=(n, 2)),
                        status=np.zeros(n, dtype=np.int32), iters=np.full(n, 5, dtype=np.int32), pred=rng.normal(size=(n, N + 1, 5)))
    return dict(table=table, x_last=x_last, steps_run=25, solves=int(sum(L)), schedule=None, trace=trace)


_REF = {}


def batch_trace(mpc_gpu, first, count, scenario="RANDOM", problem=sc.PROBLEM, max_iter=400, r_safe=None):
    """dict(simX (T + 1, B, 5), obst_traj (T + 1, B, n_obst, 4), pred (T, B, N + 1, 5), u (T, B, 2), status (T, B), iters (T, B), table, x_last, lengths (B,))
    of the one batch that holds seeds first .. first + count - 1; T >= every episode's length"""
    key = repr((mpc_gpu.BatchedMpc.default_lanes_per_stage, first, count, scenario, sorted(problem.items()), max_iter, None if r_safe is None else r_safe.tobytes()))
    if key in _REF:
        return _REF[key]
    import torch
    from mpc_gpu import _lib
    B = count
    x0, goal = np.tile(sc.START, (B, 1)), np.tile(sc.GOAL, (B, 1))
    dev = torch.device("cuda", 0)
    with mpc_gpu.BatchedMpc(max_batch=B, **problem) as m:
        N, no = m.N, m.n_obst
        obst = m.generate_scenarios(scenario, B, seed0=first)
        if r_safe is not None:
            m.set_instance_params(r_safe=r_safe)
        stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(stream):
            f64 = dict(dtype=torch.float64, device=dev); i32 = dict(dtype=torch.int32, device=dev)
            dx0, dgoal, dobst = (torch.from_numpy(a.copy()).to(dev) for a in (x0, goal, obst))
            dx0[:, 3:] = 0.0                                   # bug_compat_alias, run_episodes' default
            X = torch.zeros(B, N + 1, 5, **f64); U = torch.zeros(B, N, 2, **f64); u0 = torch.zeros(B, 2, **f64)
            status = torch.zeros(B, **i32); iters = torch.zeros(B, **i32)
            margin = torch.full((B,), float("inf"), **f64); flags = torch.zeros(B, **i32); steps = torch.zeros(B, **i32)
            s = stream.cuda_stream
            m.reset_guess_dev(B, dx0, X, U, stream=s)
            fl = _lib.STEP_SHIFT | _lib.STEP_PLANT | _lib.STEP_OBSTACLES | _lib.STEP_METRICS | _lib.STEP_RESET_ON_FAIL | _lib.STEP_ALIAS_BUG
            gen_state = m.noise_state(B, scenario, seed0=first, stream=s)
            nbuf = torch.zeros(B, no, 2, **f64)
            rec = dict(x=[dx0.clone()], obst=[dobst.clone()], X=[], u=[], status=[], iters=[])
            k = 0
            while k < max_iter:
                m.noise_draw_dev(B, gen_state, nbuf, ep_flags=flags, stream=s)
                m.closed_loop_step_dev(B, dx0, dobst, dgoal, X, U, u0, None, status, iters, nbuf, flags=fl, min_margin=margin, ep_flags=flags, ep_steps=steps,
                                       stream=s)
                k += 1
                for n, a in (("x", dx0), ("obst", dobst), ("X", X), ("u", u0), ("status", status), ("iters", iters)):
                    rec[n].append(a.clone())
                if k % 25 == 0 and int((flags & 1).min().item()) == 1:
                    break
            stream.synchronize()
            fl_h, xl = flags.cpu().numpy(), dx0.cpu().numpy()
            table = np.column_stack([(fl_h & 4) != 0, (fl_h & 1) != 0, margin.cpu().numpy(), np.linalg.norm(xl[:, :2] - goal, axis=1), steps.cpu().numpy(),
                                     (fl_h & 2) != 0]).astype(np.float64)
            out = dict(simX=torch.stack(rec["x"]).cpu().numpy(), obst_traj=torch.stack(rec["obst"]).cpu().numpy(), pred=torch.stack(rec["X"]).cpu().numpy(),
                       u=torch.stack(rec["u"]).cpu().numpy(), status=torch.stack(rec["status"]).cpu().numpy(), iters=torch.stack(rec["iters"]).cpu().numpy(),
                       table=table, x_last=xl, lengths=(table[:, 4] + table[:, 1]).astype(np.int64))
    # the yardstick against the committed path: run_episodes(record=True) on the same batch (it may stop a poll earlier or later: behind the last episode's end
    # every instance idles, so the common rows are compared and both must cover every episode)
    kw = {} if r_safe is None else dict(r_safe=r_safe)
    ref = mpc_gpu.run_episodes(x0, goal, scenario, first_seed=first, compact_from=None, record=True, max_iter=max_iter, **problem, **kw)
    T = min(k, ref["steps_run"])
    assert T >= out["lengths"].max()
    assert np.array_equal(out["table"], ref["table"]) and np.array_equal(out["x_last"], ref["x_last"])
    assert np.array_equal(out["simX"][:T + 1], ref["simX"][:T + 1]) and np.array_equal(out["obst_traj"][:T + 1], ref["obst_traj"][:T + 1])
    assert np.array_equal(out["pred"][:T], ref["pred"][:T])
    for a in out.values():
        a.setflags(write=False)
    _REF[key] = out
    return out


def assert_trace_is_column(t, bt, col, pred=True):
    """one seed's trace against column `col` of the batch: rows 0 .. L of the states, 0 .. L-1 of the step words, bit for bit"""
    L = int(bt["lengths"][col])
    assert t["u"].shape == (L, 2) and t["simX"].shape[0] == L + 1 and t["obst_traj"].shape[0] == L + 1 and t["status"].shape == (L,) and t["iters"].shape == (L,), col
    assert np.array_equal(t["simX"], bt["simX"][:L + 1, col]), col
    assert np.array_equal(t["obst_traj"], bt["obst_traj"][:L + 1, col]), col
    assert np.array_equal(t["u"], bt["u"][:L, col]), col
    assert np.array_equal(t["status"], bt["status"][:L, col]) and np.array_equal(t["iters"], bt["iters"][:L, col]), col
    if pred:
        assert np.array_equal(t["pred"], bt["pred"][:L, col]), col
    else:
        assert "pred" not in t
