"""Shared cases of the per-group record tests (test_multistart_record_host.py, test_gpu_multistart_record.py): the two phases of mpc_group_record_dev restated
in numpy (`solved`, `stepped`) over the arrays of struct mpc_group_record, made-up group words that cover the roles a group can be in (`made_up`, `fake_tail`),
a synthetic run_multistart_episodes result for multistart_record, and -- for the GPU tests -- `clone_loop`, the path that exists without the feature: the
test's own loop over the entry points that were there before it (member solve, optional predict + rollout merit, mpc_group_step_dev) with clones behind each
launch.  Imports without torch or a GPU.  No test functions here."""
import numpy as np

FIELDS = ["group_row", "len", "x", "obst", "u", "winner", "best_key", "cand_key", "cand_status", "cand_iters", "cand_u0", "cand_X"]
NEW = ("mpc_group_record_set_dev", "mpc_group_record_dev")
SOLVED, STEPPED = 0, 1

# bytes of a record by hand: 2 groups, 10 control steps, N 20, 5 obstacles, K 3.  Per group: x 11 * 5 * 8 = 440, obst 11 * 5 * 4 * 8 = 1760, u 10 * 2 * 8 = 160,
# best_key 10 * 8 = 80, cand_key 10 * 3 * 8 = 240, cand_u0 10 * 3 * 2 * 8 = 480, winner 10 * 4 = 40, cand_status + cand_iters 2 * 10 * 3 * 4 = 240, len 4
# -> 3444; cand_X 10 * 3 * 21 * 5 * 8 = 25200 -> 28644
BYTES_CASE = dict(rows=2, max_iter=10, N=20, n_obst=5, K=3, without_plans=2 * 3444, with_plans=2 * 28644)

F_SENT, I_SENT = -7.5, -7          # what the record arrays hold before a launch

# the record arrays: name -> (the trailing dimensions behind [rows], with "T" = max_steps, "T1" = max_steps + 1, "K", "no", "N1" = N + 1; dtype)
ARRAYS = dict(len=((), "i4"), x=(("T1", 5), "f8"), obst=(("T1", "no", 4), "f8"), u=(("T", 2), "f8"), winner=(("T",), "i4"), best_key=(("T",), "f8"),
              cand_key=(("T", "K"), "f8"), cand_status=(("T", "K"), "i4"), cand_iters=(("T", "K"), "i4"), cand_u0=(("T", "K", 2), "f8"),
              cand_X=(("T", "K", "N1", 5), "f8"))
# the inputs of mpc_group_record_dev: name -> (rows: "G" groups or "B" members; trailing dimensions; dtype)
INPUTS = dict(x=("G", (5,), "f8"), obst=("G", ("no", 4), "f8"), X=("B", ("N1", 5), "f8"), key=("B", (), "f8"), status=("B", (), "i4"), iters=("B", (), "i4"),
              u0=("B", (2,), "f8"), winner=("G", (), "i4"), best_key=("G", (), "f8"), best_u0=("G", (2,), "f8"), ep_flags=("G", (), "i4"), ep_steps=("G", (), "i4"))


def shape_of(tail, rows, T, K, N, no):
    d = dict(T=T, T1=T + 1, K=K, no=no, N1=N + 1)
    return (rows,) + tuple(d.get(n, n) for n in tail)


def empty_record(rows, T, K, N, no, plans=True):
    """the record arrays of `rows` rows, every word a sentinel (len too: the caller presets the rows that are owned)"""
    return {n: np.full(shape_of(tail, rows, T, K, N, no), F_SENT if dt == "f8" else I_SENT, dtype=dt) for n, (tail, dt) in ARRAYS.items()
            if plans or n != "cand_X"}


# ---------------------------------------------------------------------------------------------------------------- the rule
def solved(rec, group_row, T, inp, K):
    """phase SOLVED on the record `rec` (a dict of arrays; cand_X may be missing) and the inputs `inp`; returns new arrays, nothing given is written"""
    b = {n: v.copy() for n, v in rec.items()}
    rows = rec["len"].shape[0]
    for g, r in enumerate(np.asarray(group_row)):
        t = int(inp["ep_steps"][g])
        if r < 0 or r >= rows or (int(inp["ep_flags"][g]) & 1) or not 0 <= t < T:
            continue
        m = slice(g * K, (g + 1) * K)
        b["x"][r, t] = inp["x"][g]; b["obst"][r, t] = inp["obst"][g]
        b["cand_key"][r, t] = inp["key"][m]; b["cand_status"][r, t] = inp["status"][m]; b["cand_iters"][r, t] = inp["iters"][m]
        b["cand_u0"][r, t] = inp["u0"][m]
        if "cand_X" in b:
            b["cand_X"][r, t] = inp["X"][m]
    return b


def stepped(rec, group_row, T, inp, K):
    """phase STEPPED, likewise"""
    b = {n: v.copy() for n, v in rec.items()}
    rows = rec["len"].shape[0]
    for g, r in enumerate(np.asarray(group_row)):
        if r < 0 or r >= rows:
            continue
        now, t = int(inp["ep_steps"][g]) + (int(inp["ep_flags"][g]) & 1), int(rec["len"][r])
        if t < 0 or now <= t or now > T:
            continue
        b["winner"][r, t] = inp["winner"][g]; b["best_key"][r, t] = inp["best_key"][g]; b["u"][r, t] = inp["best_u0"][g]
        b["x"][r, now] = inp["x"][g]; b["obst"][r, now] = inp["obst"][g]
        b["len"][r] = now
    return b


PHASE = {SOLVED: solved, STEPPED: stepped}

# ---------------------------------------------------------------------------------------------------------------- made-up group words
ROLES = ("run", "idle", "reach", "budget", "unrec")


def made_up(roles, T, K, N, no, rng, spare_rows=1):
    """G = len(roles) groups in front of a member solve's group tail, and a record that fits them: `run` is in the middle of its episode, `idle` reached its goal
    earlier (bit 0 set), `reach` reaches it in this step, `budget` solves its last step (t = T - 1) without reaching it, `unrec` runs and is not recorded.  Rows
    are handed out in descending order from the last, the first `spare_rows` rows belong to nobody.  Returns (inp, group_row, rec): rec is all sentinel but the len words of owned rows,
    which hold the steps the group has behind it."""
    G = len(roles)
    inp = {}
    for n, (rows, tail, dt) in INPUTS.items():
        sh = shape_of(tail, G if rows == "G" else G * K, T, K, N, no)
        inp[n] = rng.normal(size=sh) if dt == "f8" else rng.integers(0, 5, size=sh).astype(np.int32)
    inp["iters"] = rng.integers(1, 30, size=G * K).astype(np.int32)
    steps = dict(run=min(1, T - 1), idle=max(T - 2, 0), reach=max(T - 2, 0), budget=T - 1, unrec=min(1, T - 1))
    inp["ep_steps"] = np.array([steps[r] for r in roles], dtype=np.int32)
    inp["ep_flags"] = np.array([(1 | 4 * (g % 2)) if r == "idle" else 2 * (g % 2) for g, r in enumerate(roles)], dtype=np.int32)      # bits 1, 2 end nothing
    recorded = [g for g, r in enumerate(roles) if r != "unrec"]
    R = len(recorded) + spare_rows
    group_row = np.full(G, -1, dtype=np.int32)
    group_row[recorded] = R - 1 - np.arange(len(recorded), dtype=np.int32)      # descending: no group sits in the row of its own number
    rec = empty_record(R, T, K, N, no)
    for g in recorded:
        rec["len"][group_row[g]] = inp["ep_steps"][g] + (inp["ep_flags"][g] & 1)
    return inp, group_row, rec


def fake_tail(inp, roles, K, rng):
    """what a group tail leaves of `inp` (new arrays): idle groups untouched; every other group has a winner (or -1 for every third), a key and an input, moved
    states, OVERWRITTEN member iterates, and has counted the step -- `reach` by bit 0, the others by ep_steps"""
    out = {n: v.copy() for n, v in inp.items()}
    for g, r in enumerate(roles):
        if r == "idle":
            continue
        m = slice(g * K, (g + 1) * K)
        out["winner"][g] = -1 if g % 3 == 2 else g % K
        out["best_key"][g] = np.inf if g % 3 == 2 else rng.normal()
        out["best_u0"][g] = 0.0 if g % 3 == 2 else rng.normal(size=2)
        out["x"][g] = rng.normal(size=5); out["obst"][g] = rng.normal(size=out["obst"][g].shape); out["X"][m] = rng.normal(size=out["X"][m].shape)
        if r == "reach":
            out["ep_flags"][g] |= 1
        else:
            out["ep_steps"][g] += 1
    return out


# ---------------------------------------------------------------------------------------------------------------- a synthetic result
def synthetic_result(L=(4, 7), N=6, n_obst=2, K=3, seed=5, plans=True):
    """a run_multistart_episodes result with a hand-made record of groups 1 and 3 out of 4 (lengths L): random numbers, the right shapes; stage 0 of every plan
    is the state its solve started from, as a solve leaves it; group 1 loses its second step"""
    rng = np.random.default_rng(seed)
    table = np.zeros((4, 6)); x_last = rng.normal(size=(4, 5))
    record = {}
    for g, n in zip((1, 3), L):
        table[g, 4], table[g, 1] = n - 1, 1
        simX = rng.normal(size=(n + 1, 5))
        winner = rng.integers(0, K, size=n).astype(np.int32)
        if g == 1:
            winner[1] = -1
        cand_X = rng.normal(size=(n, K, N + 1, 5))
        cand_X[:, :, 0] = simX[:n, None]
        cand_u0 = rng.normal(size=(n, K, 2))
        u = np.where((winner >= 0)[:, None], cand_u0[np.arange(n), np.maximum(winner, 0)], 0.0)
        record[g] = dict(simX=simX, obst_traj=rng.normal(size=(n + 1, n_obst, 4)), u=u, winner=winner, key=rng.normal(size=n), cand_key=rng.normal(size=(n, K)),
                         cand_status=np.zeros((n, K), dtype=np.int32), cand_iters=np.full((n, K), 5, dtype=np.int32), cand_u0=cand_u0)
        if plans:
            record[g]["cand_X"] = cand_X
    return dict(table=table, x_last=x_last, steps_run=25, solves=K * int(sum(L)), lost_steps=np.zeros(4, np.int32), switched_steps=np.zeros(4, np.int32), record=record)


# ---------------------------------------------------------------------------------------------------------------- the path without the feature
_LOOPS = {}


def clone_loop(mpc_gpu, start, goal, scenario, first_seed, problem, select_by="cost", guess_geometry=None):
    """The yardstick of the GPU tests: run_multistart_episodes' control steps through the entry points that exist without the record -- noise draw, member solve
    (closed_loop_step_dev on the members' flag words), [predict, rollout merit], mpc_group_step_dev -- on a MultiStartMpc's own tensors, with clones of the
    group's words behind the solve and behind the tail of every step.  Returns dict(record: per group what run_multistart_episodes(record=True) returns, built
    from the clones on the host; table, x_last, lost_steps, switched_steps).  Computed once per argument set, returned read-only."""
    key = repr((np.asarray(start).tobytes(), np.asarray(goal).tobytes(), scenario, first_seed, sorted((k, repr(v)) for k, v in problem.items()), select_by,
                guess_geometry))
    if key in _LOOPS:
        return _LOOPS[key]
    import torch
    from types import SimpleNamespace
    from mpc_gpu import _lib
    from mpc_gpu.episodes import _noise_source, result_table
    start, goal = np.ascontiguousarray(start, dtype=np.float64), np.ascontiguousarray(np.broadcast_to(goal, (len(start), 2)), dtype=np.float64)
    G, T = start.shape[0], problem["max_iter"]
    with mpc_gpu.MultiStartMpc(problem["N"], problem["n_obst"], problem["Tf"], scenarios=G, offsets=problem["offsets"], incumbent_margin=problem["incumbent_margin"],
                               select_by=select_by, guess_geometry=guess_geometry) as ms:
        K, m, dev = ms.K, ms.inner, ms.dev
        pre, post = [], []
        with torch.cuda.stream(ms.stream):
            s = ms.stream.cuda_stream
            f64 = dict(dtype=torch.float64, device=dev)
            x, dgoal = torch.from_numpy(start.copy()).to(dev), torch.from_numpy(goal.copy()).to(dev)
            dobst = torch.zeros(G, ms.n_obst, 4, **f64)
            m.generate_scenarios_dev(scenario, G, dobst, seed0=first_seed, stream=s)
            ms._group_arrays()
            rows = SimpleNamespace(rows=G, obst=dobst, flags=ms.ep_flags, f64=f64, gen_state=None, nbuf=None)
            draw = _noise_source(torch, m, rows, "reference", scenario, first_seed, 0, s)
            for k in range(T):
                nz = draw(k)
                if k == 0:
                    ms._load(x, dobst, dgoal)
                    ms.member_flags.copy_((ms.ep_flags & 1).repeat_interleave(K))
                    ms._seed(x, dgoal, False, s, dobst)
                m.closed_loop_step_dev(ms.B, ms._x0, ms._obst, ms._goal, ms.X, ms.U, ms.cand_u0, ms.cand_cost, ms.cand_status, ms.cand_iters,
                                       flags=_lib.STEP_METRICS, min_margin=ms._scratch_margin, ep_flags=ms.member_flags, ep_steps=ms._scratch_steps, stream=s)
                by = ms._select_key(x, dobst, dgoal, s)
                pre.append({n: t.clone() for n, t in dict(x=x, obst=dobst, key=by, status=ms.cand_status, iters=ms.cand_iters, u0=ms.cand_u0, X=ms.X,
                                                          flags=ms.ep_flags, steps=ms.ep_steps).items()})
                _lib.check(_lib.lib().mpc_group_step_dev(m._h, G, K, by.data_ptr(), ms.cand_status.data_ptr(), ms.cand_u0.data_ptr(), ms.margin, 0, x.data_ptr(),
                                                         dobst.data_ptr(), dgoal.data_ptr(), ms.offsets.data_ptr(), nz.data_ptr(), 0.1, 2.0, ms.X.data_ptr(),
                                                         ms.U.data_ptr(), ms._out, s))
                post.append({n: t.clone() for n, t in dict(x=x, obst=dobst, winner=ms.winner, key=ms.cost, u=ms.u0).items()})
            ms.stream.synchronize()
            xl = x.cpu().numpy()
            table = result_table(ms.ep_flags.cpu().numpy(), ms.min_margin.cpu().numpy(), xl, goal, ms.ep_steps.cpu().numpy())
            lost, switched = ms.lost_steps.cpu().numpy().copy(), ms.switched_steps.cpu().numpy().copy()
        N = ms.N
    pre = [{n: t.cpu().numpy() for n, t in d.items()} for d in pre]
    post = [{n: t.cpu().numpy() for n, t in d.items()} for d in post]
    record = {}
    for g in range(G):
        rows = dict(simX=[], obst_traj=[], u=[], winner=[], key=[], cand_key=[], cand_status=[], cand_iters=[], cand_u0=[], cand_X=[])
        last = None
        for k in range(T):
            if pre[k]["flags"][g] & 1:                            # idle on entry: neither solved nor stepped
                continue
            assert pre[k]["steps"][g] == len(rows["u"])           # the yardstick itself: a running group solves its steps in order
            m_ = slice(g * K, (g + 1) * K)
            rows["simX"].append(pre[k]["x"][g]); rows["obst_traj"].append(pre[k]["obst"][g])
            rows["cand_key"].append(pre[k]["key"][m_]); rows["cand_status"].append(pre[k]["status"][m_]); rows["cand_iters"].append(pre[k]["iters"][m_])
            rows["cand_u0"].append(pre[k]["u0"][m_]); rows["cand_X"].append(pre[k]["X"][m_])
            rows["u"].append(post[k]["u"][g]); rows["winner"].append(post[k]["winner"][g]); rows["key"].append(post[k]["key"][g])
            last = k
        rows["simX"].append(post[last]["x"][g]); rows["obst_traj"].append(post[last]["obst"][g])
        record[g] = {n: np.stack(v) for n, v in rows.items()}
        assert record[g]["cand_X"].shape[1:] == (K, N + 1, 5) and len(rows["u"]) == int(table[g, 4] + table[g, 1])
        for a in record[g].values():
            a.setflags(write=False)
    out = dict(record=record, table=table, x_last=xl, lost_steps=lost, switched_steps=switched)
    for a in (table, xl, lost, switched):
        a.setflags(write=False)
    _LOOPS[key] = out
    return out
