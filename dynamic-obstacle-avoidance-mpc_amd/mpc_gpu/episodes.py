"""On-device closed-loop episode harness: `RobotOcpProblem.step` + `experiments.py` semantics for a
whole batch of scenarios, one kernel launch per control step, everything resident in HBM.

Output table columns are the reference's (src/simulation/robot_ocp_problem.py:277, sliced [1:] at experiments.py:36):
    [hit, reached_goal, min_margin, dist_to_goal, iters, out_of_bounds]
and `write_experiment` stores them as `;`-separated CSV + spec JSON like experiments.py:40-43, so tooling written for the
reference's `test_data/` (evaluate_experiments.py:8-18) reads them.
"""
import json
import os
import time

import numpy as np

from . import _lib
from .solver import BOUNDS_ROW, BatchedMpc, pack_instance_bounds, pack_obstacle_mask


def run_episodes(x0, goal, obst, N=20, Tf=2.0, max_iter=400, random_move=True, init_guess_when_error=True,
                 bug_compat_alias=True, seed=0, device=0, solver=None, n_obst=5, first_seed=0, record=False, noise=None,
                 interpolate_init=False, status_log=False, compact_from=4096, r_safe=None, r_hit=None, active=None, margin_all=False, bounds=None, sqp=None, **cfg):
    """x0 (B,5), goal (B,2), obst (B,n_obst,4) -- or a scenario name ("RANDOM" | "CENTER" | "EDGE"): instance s then starts
    from the reference generator's draw for np.random.seed(first_seed + s), produced on the device (experiments.py:26-29).
    record=True also returns simX (steps+1,B,5), obst_traj (steps+1,B,n_obst,4) and pred (steps,B,N+1,5): what the reference keeps
    for its visualisation (robot_ocp_problem.py:232-240,270-276).
    noise: an array (steps, B, n_obst, 2) -> exactly these normals, control step k using noise[k] (world.reference_streams gives the sequences the
    reference's own runs consumed, per seed); "reference" -> the same sequences produced ON THE DEVICE per instance (numpy's legacy generator for seed
    first_seed + s continued behind the scenario draw: mpc_noise_init_dev / mpc_noise_draw_dev, no host upload) -- the default when `obst` is a scenario
    name, i.e. run_episodes(x0, goal, "RANDOM", first_seed=0) IS experiments.py:20-36 for seeds 0 .. B-1; "torch" (and None with explicit obstacle states)
    -> standard normals from torch's generator (`seed`).
    interpolate_init: set_initial_guess() is the straight-line variant the reference keeps commented out (robot_ocp_problem.py:293-300; spec key
    `interpolate_init` of two recorded tables) -- at the start and on every status-4 reset.
    status_log: also return, per episode, how many of its solves ended with status 2 / status 4 and the first control step with a status != 0
    (-1: none) -- `status2`, `status4`, `first_bad`.
    compact_from: batches of at least this many episodes are COMPACTED while they run -- an episode that has reached its goal idles in its wavefront slot, and
    with the reference's protocol the mean episode is 120-170 of 400 control steps long: every 25 control steps, once a quarter of the episodes in the batch
    have finished, their results are parked and the live ones move together (device-side gathers, one host read of the count).  Each episode's arithmetic is
    its own: results are those of the uncompacted run, bit for bit where an instance's result does not depend on its wavefront neighbours (one instance
    per wavefront) and to the rounding of the wavefront sums otherwise (three per wavefront).  Off with record / status_log; None: never.
    r_safe, r_hit: optional per-instance radii, (B, n_obst) or (B,) (BatchedMpc.set_instance_params): obstacle j of episode b keeps the robot
    r_safe[b, j] away and counts as hit within r_hit[b, j] (default r_safe[b, j] - (cfg.r_safe - 1.2)).  The scenario generators draw no radii (they
    are pinned to the reference's streams): drawing them is the caller's business.  Episodes with radii of their own are not compacted.
    active: optional bool (B, n_obst) (BatchedMpc.set_obstacle_mask): obstacle j exists for episode b only where active[b, j]; the absent ones still
    move (and draw their noise) but are neither solved against nor, unless margin_all, counted in the margin and the hit flag.  Masked episodes are
    not compacted.
    bounds: optional dict(bx_lo=, bx_hi=, bu_lo=, bu_hi=) of per-instance box bounds, (B, 4) / (B, 2) or one row for all (BatchedMpc.set_instance_bounds):
    episode b is solved inside its own actuator and speed limits.  Episodes with bounds of their own are not compacted.
    sqp: optional (max_iter, step_tol) (BatchedMpc.set_sqp): every control step runs up to max_iter SQP iterations in its one launch.  Compaction stays on:
    the setting is per handle, not per episode.
    Returns dict(table (B,6), x_last (B,5), steps_run, solves)."""
    import torch
    x0 = np.ascontiguousarray(x0, dtype=np.float64); B = x0.shape[0]
    scenario_name = obst if isinstance(obst, str) else None
    if interpolate_init and bug_compat_alias:
        import warnings
        warnings.warn("interpolate_init with bug_compat_alias=True: the straight-line guess is built from a plant state whose v, omega the aliasing defect has "
                      "zeroed; the two recorded `interpolate_init` tables replay with bug_compat_alias=False (tests/test_gpu_replay.py)", stacklevel=2)
    if scenario_name is not None:
        if noise is None and random_move:
            noise = "reference"
            if seed != 0:
                raise ValueError("`seed` selects torch's generator, which a scenario name does not use: the obstacle noise is the reference's own numpy stream "
                                 "per instance (first_seed + s).  Vary first_seed, or pass noise='torch' to draw from torch's generator with this seed")
        with BatchedMpc(N, n_obst, Tf, max_batch=B, device=device) as g:
            obst = g.generate_scenarios(obst, B, seed0=first_seed)
    obst = np.ascontiguousarray(obst, dtype=np.float64); n_obst = obst.shape[1]
    goal = np.ascontiguousarray(np.broadcast_to(goal, (B, 2)), dtype=np.float64)
    dev = torch.device("cuda", device)
    m = solver or BatchedMpc(N, n_obst, Tf, max_batch=B, device=device, **cfg)
    own_radii = r_safe is not None or r_hit is not None
    if own_radii:
        m.set_instance_params(r_safe=r_safe, r_hit=r_hit)
    own_mask = active is not None
    if own_mask:
        m.set_obstacle_mask(np.asarray(active))
    own_bounds = bounds is not None
    if own_bounds:
        m.set_instance_bounds(**bounds)
    own_sqp = sqp is not None
    if own_sqp:
        m.set_sqp(*sqp)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        t = lambda a: torch.from_numpy(a.copy()).to(dev)
        dx0, dgoal, dobst = t(x0), t(goal), t(obst)
        if bug_compat_alias:                      # set_initial_guess() aliases self.x0 and zeroes v, omega (defect D2)
            dx0[:, 3:] = 0.0
        X = torch.zeros(B, N + 1, 5, dtype=torch.float64, device=dev); U = torch.zeros(B, N, 2, dtype=torch.float64, device=dev)
        status = torch.zeros(B, dtype=torch.int32, device=dev); iters = torch.zeros(B, dtype=torch.int32, device=dev)
        margin = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
        flags = torch.zeros(B, dtype=torch.int32, device=dev); steps = torch.zeros(B, dtype=torch.int32, device=dev)
        s = stream.cuda_stream
        if interpolate_init:
            m.reset_guess_interp_dev(B, dx0, dgoal, X, U, stream=s)
        else:
            m.reset_guess_dev(B, dx0, X, U, stream=s)        # set_initial_guess() at the start of step(), :180
        fl = _lib.STEP_SHIFT | _lib.STEP_PLANT | _lib.STEP_OBSTACLES | _lib.STEP_METRICS
        if init_guess_when_error:
            fl |= _lib.STEP_RESET_ON_FAIL | (_lib.STEP_ALIAS_BUG if bug_compat_alias else 0) | (_lib.STEP_INTERP_GUESS if interpolate_init else 0)
        if own_mask and margin_all:
            fl |= _lib.STEP_MARGIN_ALL
        if status_log:
            n2 = torch.zeros(B, dtype=torch.int32, device=dev); n4 = torch.zeros(B, dtype=torch.int32, device=dev)
            first_bad = torch.full((B,), -1, dtype=torch.int32, device=dev)
        gen = torch.Generator(device=dev); gen.manual_seed(seed)
        dnoise = None
        gen_state, nbuf = None, None
        if isinstance(noise, str) and noise == "torch":
            noise = None
        if isinstance(noise, str):
            if noise != "reference" or scenario_name is None:
                raise ValueError("noise='reference' continues the generator of a scenario draw: pass the scenario name as `obst`")
            if random_move:
                gen_state = m.noise_state(B, scenario_name, seed0=first_seed, stream=s)
                nbuf = torch.zeros(B, n_obst, 2, dtype=torch.float64, device=dev)
        elif noise is not None and random_move:
            noise = np.ascontiguousarray(noise, dtype=np.float64)
            if noise.shape[1:] != (B, n_obst, 2) or noise.shape[0] < max_iter:
                raise ValueError(f"noise must be (>= {max_iter}, {B}, {n_obst}, 2), got {noise.shape}")
            dnoise = torch.from_numpy(noise).to(dev)
        k = 0
        # compaction of finished episodes (compact_from): results of parked episodes live in full-size arrays, `ids` maps the live batch to them
        compact = compact_from is not None and B >= compact_from and not record and not status_log and not own_radii and not own_mask and not own_bounds
        B0 = B
        if compact:
            ids = torch.arange(B, device=dev)
            full = dict(margin=margin.clone(), flags=flags.clone(), steps=steps.clone(), x=dx0.clone())
        rec_x, rec_o, rec_p = [dx0.clone()], [dobst.clone()], []
        # "every instance has reached its goal" without stalling the queue: every 25 control steps the flag goes to pinned host memory behind an event,
        # and is looked at only once that event has passed (so the loop runs at most ~25 steps longer than it has to -- on idle instances, which cost nothing)
        done_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        done_event = None
        while k < max_iter:
            if not random_move:
                nz = None
            elif gen_state is not None:
                m.noise_draw_dev(B, gen_state, nbuf, ep_flags=flags, stream=s); nz = nbuf
            elif dnoise is not None:
                nz = dnoise[k] if B == B0 else dnoise[k][ids]
            else:
                nz = torch.randn(B, n_obst, 2, dtype=torch.float64, device=dev, generator=gen)
            m.closed_loop_step_dev(B, dx0, dobst, dgoal, X, U, None, None, status, iters, nz, flags=fl,
                                   min_margin=margin, ep_flags=flags, ep_steps=steps, stream=s)
            if status_log:      # (an episode that has reached its goal idles: its status word keeps the last solve's value and is not counted again)
                live = (steps + (flags & 1)) > k
                n2 += (live & (status == 2)).int(); n4 += (live & (status == 4)).int()
                first_bad = torch.where(live & (status != 0) & (first_bad < 0), torch.full_like(first_bad, k), first_bad)
            k += 1
            if record:      # X holds the shifted prediction: stage j of the solve is X[j - 1], stage N is kept (:253-258)
                rec_x.append(dx0.clone()); rec_o.append(dobst.clone()); rec_p.append(X.clone())
            if done_event is not None and done_event.query():
                if int(done_host[0]) == 1:
                    break
                done_event = None
            if compact and k % 25 == 0:
                live = (flags & 1) == 0
                n_live = int(live.sum().item())                 # (the one host read: at these batch sizes 25 control steps take tens of milliseconds)
                if n_live == 0:
                    break
                if n_live <= 0.75 * B:
                    park = ids[~live]
                    full["margin"][park] = margin[~live]; full["flags"][park] = flags[~live]; full["steps"][park] = steps[~live]; full["x"][park] = dx0[~live]
                    take = lambda a: a[live].contiguous()
                    ids, dx0, dgoal, dobst, X, U = take(ids), take(dx0), take(dgoal), take(dobst), take(X), take(U)
                    status, iters, margin, flags, steps = take(status), take(iters), take(margin), take(flags), take(steps)
                    if gen_state is not None:
                        gen_state, nbuf = take(gen_state), take(nbuf)
                    B = n_live
                continue
            if k % 25 == 0 and done_event is None:
                done_host.copy_((flags & 1).min().to(torch.int32).reshape(1), non_blocking=True)
                done_event = torch.cuda.Event(); done_event.record(stream)
        stream.synchronize()
        if compact:
            full["margin"][ids] = margin; full["flags"][ids] = flags; full["steps"][ids] = steps; full["x"][ids] = dx0
            margin, flags, steps, dx0 = full["margin"], full["flags"], full["steps"], full["x"]
        fl_h = flags.cpu().numpy(); xl = dx0.cpu().numpy()
        table = np.column_stack([(fl_h & 4) != 0, (fl_h & 1) != 0, margin.cpu().numpy(),
                                 np.linalg.norm(xl[:, :2] - goal, axis=1), steps.cpu().numpy(), (fl_h & 2) != 0]).astype(np.float64)
        extra = {}
        if record:
            extra = dict(simX=torch.stack(rec_x).cpu().numpy(), obst_traj=torch.stack(rec_o).cpu().numpy(), pred=torch.stack(rec_p).cpu().numpy())
        if status_log:
            extra.update(status2=n2.cpu().numpy(), status4=n4.cpu().numpy(), first_bad=first_bad.cpu().numpy())
    if solver is None:
        m.close()
    else:                            # (a caller's solver leaves as it came)
        if own_radii:
            m.set_instance_params()
        if own_mask:
            m.set_obstacle_mask(None)
        if own_bounds:
            m.set_instance_bounds()
        if own_sqp:
            m.set_sqp()
    return dict(table=table, x_last=xl, steps_run=k, solves=int(steps.sum().item()) + int((fl_h & 1).sum()), **extra)


def refill_schedule(lengths, slots):
    """The slot-order assignment of mpc_episode_refill_dev as a pure-numpy model.  lengths[k]: the fused control steps seed index k runs (a table row's
    `iters + reached`, >= 1); slots: the slot count asked for (min(slots, count) are used).  In front of control step t every slot whose episode has
    ended takes the lowest seed index not started yet, lowest slot first.  Returns dict(slot (count,), start (count,): the slot and the control
    step at which each seed starts; steps: the control steps until the last episode ends = the fused steps a sweep launches)."""
    import heapq
    lengths = np.asarray(lengths)
    if lengths.ndim != 1 or not np.issubdtype(lengths.dtype, np.number) or (lengths.size and (lengths != np.floor(lengths)).any()):
        raise ValueError("lengths must be a 1-d array of whole step counts")
    lengths = lengths.astype(np.int64)
    if (lengths < 1).any():
        raise ValueError("every episode runs at least one fused control step")
    if int(slots) < 1:
        raise ValueError("slots must be >= 1")
    count = lengths.size
    S = min(int(slots), count)
    slot = np.zeros(count, dtype=np.int64); start = np.zeros(count, dtype=np.int64)
    free = [(0, s) for s in range(S)]          # (control step at which the slot is free, slot): the heap pops the earliest step, then the lowest slot
    heapq.heapify(free)
    steps = 0
    for k in range(count):
        t, s = heapq.heappop(free)
        slot[k], start[k] = s, t
        steps = max(steps, t + int(lengths[k]))
        heapq.heappush(free, (t + int(lengths[k]), s))
    return dict(slot=slot, start=start, steps=int(steps))


def _sweep_arguments(start, goal, scenario, seeds, slots, max_iter, poll_every):
    """run_seed_sweep's arguments, checked on the host before anything touches a device: (first, count, start rows, goal rows, per_seed)"""
    if not isinstance(scenario, str):
        raise ValueError("a sweep is defined by a scenario name (\"RANDOM\" | \"CENTER\" | \"EDGE\"): explicit obstacle states are run_episodes' business")
    if scenario not in BatchedMpc.SCENARIOS:
        raise ValueError(f"unknown scenario {scenario!r}: one of {sorted(BatchedMpc.SCENARIOS)}")
    if isinstance(seeds, range):
        if seeds.step != 1:
            raise ValueError("seeds must be consecutive: a range with step 1, or (first, count)")
        first, count = seeds.start, len(seeds)
    else:
        try:
            first, count = seeds
            first, count = int(first), int(count)
        except (TypeError, ValueError):
            raise ValueError("seeds must be (first, count) or a range with step 1") from None
    if count < 1 or first < 0 or first + count > 2 ** 32:
        raise ValueError("seeds must name at least one numpy seed in [0, 2^32)")
    if count >= 2 ** 31:
        raise ValueError("a sweep holds fewer than 2^31 seeds")
    if int(slots) != slots or int(slots) < 1:
        raise ValueError("slots must be a whole number >= 1")
    if int(max_iter) < 1 or int(poll_every) < 1:
        raise ValueError("max_iter and poll_every must be >= 1")
    start = np.ascontiguousarray(start, dtype=np.float64); goal = np.ascontiguousarray(goal, dtype=np.float64)
    per = []
    for name, a, cols in (("start", start, 5), ("goal", goal, 2)):
        if a.shape == (cols,) or a.shape == (1, cols):
            per.append(False)
        elif a.ndim == 2 and a.shape[1] == cols:
            if a.shape[0] != count:
                raise ValueError(f"per-seed {name} has {a.shape[0]} rows for {count} seeds")
            per.append(True)
        else:
            raise ValueError(f"{name} must be ({cols},) or (count, {cols}), got {a.shape}")
    per_seed = any(per)
    rows = count if per_seed else 1
    start = np.array(np.broadcast_to(start.reshape(-1, 5), (rows, 5)), order="C"); goal = np.array(np.broadcast_to(goal.reshape(-1, 2), (rows, 2)), order="C")      # (copies: writable)
    return first, count, start, goal, per_seed


# mpc_default_config's box bounds (robot_ocp_problem.py:91-96): what a handle run_seed_sweep creates itself holds unless **cfg overrides them -- known here
# so that per-seed bounds are checked against the other side before a handle exists (tests/test_sweep_features_host.py holds them to the library's)
DEFAULT_BOUNDS = dict(bx_lo=(-7.0, -7.0, -10.0, -10.0), bx_hi=(7.0, 7.0, 10.0, 10.0), bu_lo=(-8.0, -8.0), bu_hi=(8.0, 8.0))


def ring_model(schedule_start, capacity, every):
    """Which seeds a sweep's ring serves, as a pure-numpy model of mpc_episode_ring_fill_dev.  schedule_start[k]: the control step at which seed index k starts
    (refill_schedule's `start`, run_seed_sweep's schedule[:, 1]); capacity: ring entries; every: the ring is filled in front of the refill of the control steps
    t % every == 0.  The fill at step t_f seeds the indices [handed(t_f), handed(t_f) + capacity), handed(t) being the number of seeds started before t; so seed
    k, started at step t, is served from the ring when k < handed(t_f) + capacity with t_f the last fill step <= t, and seeds in place otherwise.
    Returns int32 (count,): 1 ring, 0 in place -- run_seed_sweep's `seed_src`."""
    start = np.asarray(schedule_start)
    if start.ndim != 1 or (start.size and (start < 0).any()):
        raise ValueError("schedule_start must be a 1-d array of control steps >= 0")
    if int(capacity) < 1 or int(every) < 1:
        raise ValueError("capacity and every must be >= 1")
    start = start.astype(np.int64)
    t_f = (start // int(every)) * int(every)
    handed = np.searchsorted(np.sort(start), t_f, side="left")          # seeds started before t_f
    return (np.arange(start.size) < handed + int(capacity)).astype(np.int32)


def _sweep_features(count, n_obst, handle_cfg, r_safe=None, r_hit=None, W=None, We=None, active=None, margin_all=False, bounds=None, status_log=False,
                    ring=None, ring_every=None, poll_every=25):
    """run_seed_sweep's per-seed arguments, checked on the host by the setters' own rules before anything touches a device.  handle_cfg: an object with the
    handle's bx_lo, bx_hi, bu_lo, bu_hi (an MpcConfig, or a dict over DEFAULT_BOUNDS).  Returns dict(W, We, r_safe, r_hit (float64 (count, .) or None),
    mask (int32 words (count,) or None), bounds (float64 (count, 12) or None), margin_all, status_log, ring (capacity or None), ring_every)."""
    out = dict(margin_all=bool(margin_all), status_log=bool(status_log))
    for name, a, cols, low, open_ in (("W", W, 6, 0.0, False), ("We", We, 4, 0.0, False), ("r_safe", r_safe, n_obst, 0.0, True), ("r_hit", r_hit, n_obst, 0.0, True)):
        if a is not None:
            a = np.asarray(a, dtype=np.float64)
            if a.ndim == 1 and name in ("r_safe", "r_hit"):
                a = np.repeat(a[:, None], n_obst, axis=1)
            if a.ndim != 2 or a.shape[1] != cols:
                raise ValueError(f"{name} must be (count, {cols})" + (" or (count,)" if name in ("r_safe", "r_hit") else "") + f", got {a.shape}")
            if a.shape[0] != count:
                raise ValueError(f"per-seed {name} has {a.shape[0]} rows for {count} seeds")
            if not np.isfinite(a).all() or not ((a > low) if open_ else (a >= low)).all():
                raise ValueError(f"per-seed {name} must be finite and " + ("> 0" if open_ else ">= 0"))
            a = np.ascontiguousarray(a)
        out[name] = a
    out["mask"] = None
    if active is not None:
        a = np.asarray(active)
        if a.ndim != 2 or a.shape[1] != n_obst:
            raise ValueError(f"active must be (count, {n_obst}), got {a.shape}: a mask has no bit at or above n_obst")
        if a.shape[0] != count:
            raise ValueError(f"per-seed active has {a.shape[0]} rows for {count} seeds")
        out["mask"] = pack_obstacle_mask(a).view(np.int32)
    out["bounds"] = None
    if bounds is not None:
        if not isinstance(bounds, dict) or set(bounds) - {n for n, _, _ in BOUNDS_ROW}:
            raise ValueError("bounds must be a dict with keys among bx_lo, bx_hi, bu_lo, bu_hi")
        given = {n: v for n, v in bounds.items() if v is not None}
        if not given:
            raise ValueError("bounds names no group")
        for n, v in given.items():
            v = np.asarray(v, dtype=np.float64)
            if v.ndim == 2 and v.shape[0] != count:
                raise ValueError(f"per-seed {n} has {v.shape[0]} rows for {count} seeds")
            if not np.isfinite(v).all():
                raise ValueError(f"bounds: {n} entries must be finite")
        get = (lambda n: handle_cfg[n]) if isinstance(handle_cfg, dict) else (lambda n: list(getattr(handle_cfg, n)))
        own = type("Cfg", (), {n: get(n) for n, _, _ in BOUNDS_ROW})
        tab = pack_instance_bounds(own, count, **given)
        at = {n: (c0, c) for n, c0, c in BOUNDS_ROW}
        for lo, hi in (("bu_lo", "bu_hi"), ("bx_lo", "bx_hi")):
            if not (tab[:, at[lo][0]:at[lo][0] + at[lo][1]] < tab[:, at[hi][0]:at[hi][0] + at[hi][1]]).all():
                raise ValueError(f"bounds: {lo} must be below {hi} in every component (against the handle's value where one side is missing)")
        out["bounds"] = tab
    if ring is not None and (isinstance(ring, bool) or int(ring) != ring or int(ring) < 1):
        raise ValueError("ring must be None (off) or a capacity >= 1")
    ring_every = poll_every if ring_every is None else ring_every
    if int(ring_every) != ring_every or int(ring_every) < 1:
        raise ValueError("ring_every must be a whole number >= 1")
    out["ring"] = None if ring is None else int(ring); out["ring_every"] = int(ring_every)
    return out


def trace_bytes(rows, max_iter, N, n_obst, pred=True):
    """device bytes of a sweep's trace arrays (mpc_episode_trace): per traced seed x (max_iter + 1, 5), obst (max_iter + 1, n_obst, 4), u (max_iter, 2) and,
    with pred, pred (max_iter, N + 1, 5) in float64, status and iters (max_iter,) and one len word in int32"""
    rows, T, N, n_obst = int(rows), int(max_iter), int(N), int(n_obst)
    per_row = 8 * ((T + 1) * 5 + (T + 1) * n_obst * 4 + T * 2 + (T * (N + 1) * 5 if pred else 0)) + 4 * (2 * T + 1)
    return rows * per_row


def _sweep_trace(count, max_iter, N, n_obst, trace=None, trace_pred=True, trace_max_bytes=2 ** 31):
    """run_seed_sweep's trace arguments, checked on the host before anything touches a device.  Returns None (no trace) or dict(seeds: the traced seed indices
    (rows,) in the order given, seed_row: int32 (count,) = the row of each seed index or -1, pred, bytes)."""
    if trace is None or trace is False:
        return None
    if not isinstance(trace_pred, (bool, np.bool_)):
        raise ValueError("trace_pred must be True or False")
    if isinstance(trace_max_bytes, (bool, np.bool_)) or not isinstance(trace_max_bytes, (int, np.integer)) or trace_max_bytes < 0:
        raise ValueError("trace_max_bytes must be a whole number of bytes >= 0")
    if trace is True:
        seeds = np.arange(count, dtype=np.int64)
    else:
        if isinstance(trace, (str, bytes, dict, set, frozenset)) or not hasattr(trace, "__len__"):
            raise ValueError("trace must be None, True or a sequence of seed indices in 0 .. count-1")
        try:
            a = np.asarray(trace)
        except Exception:
            raise ValueError("trace must be None, True or a sequence of seed indices in 0 .. count-1") from None
        if a.ndim != 1 or a.size == 0 or a.dtype.kind not in "iu":
            raise ValueError(f"trace must be a non-empty 1-d sequence of whole seed indices (0 .. count-1, not seeds), got {a.dtype} {a.shape}")
        if (a < 0).any() or (a >= count).any():
            raise ValueError(f"trace holds a seed index outside 0 .. {count - 1}: {a[(a < 0) | (a >= count)][0]}")
        seeds = a.astype(np.int64)
        if np.unique(seeds).size != seeds.size:
            raise ValueError("trace names a seed index twice (every traced seed owns one row)")
    need = trace_bytes(seeds.size, max_iter, N, n_obst, pred=bool(trace_pred))
    if need > trace_max_bytes:
        raise ValueError(f"trace: the arrays of {seeds.size} seeds x {int(max_iter)} control steps take {need} bytes, more than trace_max_bytes = {int(trace_max_bytes)}: "
                         "trace fewer seeds" + (" or pass trace_pred=False (the predicted horizons are most of it)" if trace_pred else ""))
    seed_row = np.full(count, -1, dtype=np.int32)
    seed_row[seeds] = np.arange(seeds.size, dtype=np.int32)
    return dict(seeds=seeds, seed_row=seed_row, pred=bool(trace_pred), bytes=need)


def run_seed_sweep(start, goal, scenario, seeds, slots, N=20, Tf=2.0, n_obst=5, max_iter=400, random_move=True, init_guess_when_error=True,
                   bug_compat_alias=True, interpolate_init=False, sqp=None, device=0, solver=None, poll_every=25, r_safe=None, r_hit=None, W=None, We=None,
                   active=None, margin_all=False, bounds=None, status_log=False, ring=None, ring_every=None, trace=None, trace_pred=True,
                   trace_max_bytes=2 ** 31, **cfg):
    """experiments.py:20-36 for MORE SEEDS THAN SLOTS: the seeds stream through min(slots, count) slots, and a slot whose episode has ended (goal reached,
    robot_ocp_problem.py:247-250, or max_iter control steps spent) starts the next seed on the device, in front of the next fused control step
    (mpc_episode_refill_dev: no host read, no gather, every slot stays live until the seeds run out).  Seed index k is instance k of
    run_episodes(start, goal, scenario, first_seed=first): the same scenario draw, noise stream, initial guess and control steps -- the table rows are
    those of that one batch, bit for bit where an instance has a wavefront to itself and to the rounding of the wavefront sums where three share one.
    scenario: "RANDOM" | "CENTER" | "EDGE".  seeds: (first, count) or a range with step 1.  start (5,), goal (2,): one row for all seeds, or (count, 5) /
    (count, 2): one per seed.  random_move, init_guess_when_error, bug_compat_alias, interpolate_init, sqp: as run_episodes.
    poll_every: every poll_every control steps the live-slot count goes to pinned host memory behind an event, and is looked at one poll later (the queue
    never drains, and the loop ends at most two polls behind the last episode -- on idle slots); 1: after every refill, blocking, which also records the
    schedule.  The loop launches at most ceil(count / slots) * max_iter + poll_every control steps whatever the device returns.
    PER SEED, as run_episodes takes them per instance (row k belongs to seed index k; the refill copies it into the slot that starts k, mpc_set_refill_tables_dev;
    validated here by the setters' rules before anything touches a device): r_safe, r_hit (count, n_obst) or (count,) -- r_hit defaults to
    r_safe - (cfg.r_safe - 1.2); W (count, 6), We (count, 4) cost weights; active bool (count, n_obst) with margin_all; bounds dict(bx_lo=, bx_hi=, bu_lo=,
    bu_hi=) of (count, 4) / (count, 2) rows or one row for all.  The feature kernels run one instance per wavefront, so the rows are those of
    run_episodes on one batch with the same arrays, bit for bit.
    status_log: per seed, how many of its solves ended with status 2 / status 4 and its first control step with a status != 0 (-1: none), counted on the
    device behind every fused step (mpc_episode_status_log_dev) -- `status2`, `status4`, `first_bad`, as run_episodes(status_log=True) returns them.
    ring: None (off, the default) or the capacity of a ring of seeded episodes (mpc_episode_ring_dev): every ring_every control steps (default poll_every;
    step 0 included) ONE launch seeds the next `ring` seed indices, and a slot that starts a seed copies its generator state and obstacle draw from the ring
    instead of seeding numpy's generator serially inside the refill.  The ring is a cache validated by tags: an index it does not hold is seeded in place,
    and the rows are those of the sweep without a ring, bit for bit.
    Returns dict(table (count, 6), x_last (count, 5), steps_run, solves, schedule): table as run_episodes builds it; steps_run the fused steps
    launched -- with T = refill_schedule(table[:, 4] + table[:, 1], slots)["steps"] that is T for poll_every = 1 and (ceil(T / poll_every) + 1) * poll_every
    otherwise (capped by the loop bound); schedule (count, 2) = slot and control step at
    which each seed started (poll_every = 1; None otherwise), which is refill_schedule's slot / start.  With status_log: status2, status4, first_bad (count,).
    With ring and poll_every = 1: seed_src (count,) = 1 where the seed came from the ring, 0 where it was seeded in place = ring_model(schedule[:, 1], ring, ring_every).
    trace: None (off, the default), True (every seed) or a sequence of seed INDICES in 0 .. count-1 without duplicates: what run_episodes(record=True) keeps, per
    traced seed and recorded on the device (mpc_episode_trace_set_dev / mpc_episode_trace_dev: two small launches per control step, in front of and behind the
    fused step, which then also writes u*).  `trace` in the result is a dict keyed by seed index; with L = the seed's control steps (= table[k, 4] + table[k, 1])
    each value holds simX (L + 1, 5), obst_traj (L + 1, n_obst, 4), u (L, 2), status (L,), iters (L,) and, unless trace_pred=False, pred (L, N + 1, 5): the
    iterate behind each step as run_episodes records it.  sweep_record(result, k) puts one seed into run_episodes(record=True)'s layout for visualisation_inputs.
    The arrays take trace_bytes(rows, max_iter, N, n_obst, trace_pred) device bytes (90 kB per seed without pred and 426 kB with, at max_iter 400, N 20 and
    5 obstacles); above trace_max_bytes the call is refused on the host.  The rows are those of the sweep without a trace, bit for bit.
    Not offered: `record` as an argument (trace= is the sweep's form of it: rows of unequal length per seed, not a batch), a per-seed stage reference, host
    noise, PipelinedMpc."""
    not_offered = sorted(set(cfg) & {"record", "noise", "seed", "first_seed", "compact_from"})
    if not_offered:
        raise TypeError(f"run_seed_sweep has no argument {not_offered[0]!r}: it is run_episodes' (a sweep would need it per seed)")
    first, count, start, goal, per_seed = _sweep_arguments(start, goal, scenario, seeds, slots, max_iter, poll_every)
    handle_cfg = solver.cfg if solver is not None else {n: tuple(cfg.get(n, v)) for n, v in DEFAULT_BOUNDS.items()}
    ft = _sweep_features(count, solver.n_obst if solver is not None else int(n_obst), handle_cfg, r_safe=r_safe, r_hit=r_hit, W=W, We=We, active=active,
                         margin_all=margin_all, bounds=bounds, status_log=status_log, ring=ring, ring_every=ring_every, poll_every=poll_every)
    tr = _sweep_trace(count, max_iter, solver.N if solver is not None else int(N), solver.n_obst if solver is not None else int(n_obst), trace=trace,
                      trace_pred=trace_pred, trace_max_bytes=trace_max_bytes)
    import torch
    S = min(int(slots), count); max_iter = int(max_iter); poll_every = int(poll_every)
    if interpolate_init and bug_compat_alias:
        import warnings
        warnings.warn("interpolate_init with bug_compat_alias=True: the straight-line guess is built from a plant state whose v, omega the aliasing defect has "
                      "zeroed; the two recorded `interpolate_init` tables replay with bug_compat_alias=False (tests/test_gpu_replay.py)", stacklevel=2)
    dev = torch.device("cuda", device)
    m = solver or BatchedMpc(N, n_obst, Tf, max_batch=S, device=device, **cfg)
    N, n_obst = m.N, m.n_obst
    if sqp is not None:
        m.set_sqp(*sqp)
    stream = torch.cuda.Stream(device=dev)
    own_params = any(ft[n] is not None for n in ("W", "We", "r_safe", "r_hit"))
    own_mask, own_bounds, own_tables, own_trace = ft["mask"] is not None, ft["bounds"] is not None, False, False
    with torch.cuda.stream(stream):
        f64 = dict(dtype=torch.float64, device=dev); i32 = dict(dtype=torch.int32, device=dev)
        dstart, dgoal_rows = torch.from_numpy(start).to(dev), torch.from_numpy(goal).to(dev)
        dx0 = torch.zeros(S, 5, **f64); dgoal = torch.zeros(S, 2, **f64); dobst = torch.zeros(S, n_obst, 4, **f64)
        X = torch.zeros(S, N + 1, 5, **f64); U = torch.zeros(S, N, 2, **f64)
        status = torch.zeros(S, **i32); iters = torch.zeros(S, **i32)
        margin = torch.full((S,), float("inf"), **f64)
        flags = torch.ones(S, **i32); steps = torch.zeros(S, **i32)          # every slot "finished" and without a seed: the first refill fills them all
        slot_seed = torch.full((S,), -1, **i32); cursor = torch.zeros(2, **i32)
        gen_state = torch.zeros(S, _lib.lib().mpc_noise_state_words(), **i32)
        nbuf = torch.zeros(S, n_obst, 2, **f64) if random_move else None
        res_f = torch.full((count, 6), float("nan"), **f64); res_i = torch.full((count, 2), -1, **i32)
        s = stream.cuda_stream
        fl = _lib.STEP_SHIFT | _lib.STEP_PLANT | _lib.STEP_OBSTACLES | _lib.STEP_METRICS
        if init_guess_when_error:
            fl |= _lib.STEP_RESET_ON_FAIL | (_lib.STEP_ALIAS_BUG if bug_compat_alias else 0) | (_lib.STEP_INTERP_GUESS if interpolate_init else 0)
        if own_mask and ft["margin_all"]:
            fl |= _lib.STEP_MARGIN_ALL
        rf = (_lib.REFILL_ALIAS_BUG if bug_compat_alias else 0) | (_lib.REFILL_INTERP_GUESS if interpolate_init else 0) | (_lib.REFILL_DRAW_NOISE if random_move else 0)
        # per-seed tables: the sources (count rows) and the per-slot arrays the solve reads in place (max_batch rows, preset with the handle's own values: a
        # slot that never gets a seed holds valid numbers), registered with the _dev setters; the refill copies row k into the slot that starts k
        MB = m.max_batch
        tabs = {}
        if own_params:
            r_hit_own = 1.0 + 0.2                               # o.r + R_ROBOT: the fused step's hit radius (mpc_closed_loop_step_dev)
            preset = dict(W=list(m.cfg.W), We=list(m.cfg.We), r_safe=[m.cfg.r_safe] * n_obst, r_hit=[r_hit_own] * n_obst)
            slot = {}
            for name in ("W", "We", "r_safe", "r_hit"):
                if ft[name] is not None:
                    tabs[name] = torch.from_numpy(ft[name]).to(dev)
                    slot[name] = tabs["slot_" + name] = torch.tensor(preset[name], **f64).repeat(MB, 1).contiguous()
            m.set_instance_params(W=slot.get("W"), We=slot.get("We"), r_safe=slot.get("r_safe"), r_hit=slot.get("r_hit"))
        if own_mask:
            tabs["mask"] = torch.from_numpy(ft["mask"].copy()).to(dev)
            tabs["slot_mask"] = torch.full((MB,), int(np.array([(1 << n_obst) - 1], dtype=np.uint32).view(np.int32)[0]), **i32)
            m.set_obstacle_mask(tabs["slot_mask"])
        if own_bounds:
            tabs["bounds"] = torch.from_numpy(ft["bounds"]).to(dev)
            tabs["slot_bounds"] = torch.from_numpy(pack_instance_bounds(m.cfg, MB)).to(dev)
            m.set_instance_bounds_dev(tabs["slot_bounds"])
        if ft["status_log"]:
            tabs["log"] = torch.tensor([0, 0, -1, 0], **i32).repeat(S, 1).contiguous()
            tabs["res_log"] = torch.full((count, 3), -1, **i32)
        if tabs:
            m.set_refill_tables_dev(**tabs); own_tables = True
        ring_cap, ring_every = ft["ring"], ft["ring_every"]
        seed_src = None
        if ring_cap is not None:
            ring_state = torch.zeros(ring_cap, gen_state.shape[1], **i32); ring_obst = torch.zeros(ring_cap, n_obst, 4, **f64)
            ring_tag = torch.full((ring_cap,), -1, **i32); seed_src = torch.full((count,), -1, **i32)
            m.episode_ring_dev(ring_cap, ring_state, ring_obst, ring_tag, seed_src)
        tarr, u0 = None, None
        if tr is not None:          # the per-seed rows (mpc_episode_trace): row r belongs to seed index tr["seeds"][r]
            R = tr["seeds"].size
            tarr = dict(seed_row=torch.from_numpy(tr["seed_row"]).to(dev), slot_state=torch.tensor([-1, 0], **i32).repeat(S, 1).contiguous(),
                        len=torch.zeros(R, **i32), x=torch.zeros(R, max_iter + 1, 5, **f64), obst=torch.zeros(R, max_iter + 1, n_obst, 4, **f64),
                        u=torch.zeros(R, max_iter, 2, **f64), status=torch.zeros(R, max_iter, **i32), iters=torch.zeros(R, max_iter, **i32),
                        pred=torch.zeros(R, max_iter, N + 1, 5, **f64) if tr["pred"] else None)
            u0 = torch.zeros(S, 2, **f64)
            m.episode_trace_set_dev(R, max_iter, **tarr); own_trace = True
        bound = -(-count // S) * max_iter + poll_every
        schedule = np.full((count, 2), -1, dtype=np.int64) if poll_every == 1 else None
        seen = np.full(S, -1, dtype=np.int64)
        live_host = torch.full((1,), -1, dtype=torch.int32).pin_memory()
        live_event = None
        k = 0
        try:
            while True:
                if ring_cap is not None and k % ring_every == 0:
                    m.episode_ring_fill_dev(scenario, first, count, cursor, stream=s)
                m.episode_refill_dev(S, scenario, first, count, max_iter, dstart, dgoal_rows, per_seed, dx0, dobst, dgoal, X, U, margin, flags, steps,
                                     gen_state, nbuf, slot_seed, cursor, res_f, res_i, flags=rf, stream=s)
                if poll_every == 1:
                    now = slot_seed.cpu().numpy()              # (blocking: this is the mode that records the schedule, not the one that is timed)
                    new = (now != seen) & (now >= 0)
                    schedule[now[new], 0] = np.nonzero(new)[0]; schedule[now[new], 1] = k
                    seen = now
                    if int(cursor[1].item()) == 0:
                        break
                elif k % poll_every == 0:
                    # the count of the poll before this one, which the device passed long ago: the host stays at most two polls ahead of the device (no idle
                    # steps by the hundred behind the end of the sweep) and the device always has a poll's worth of steps queued (it never waits for the host)
                    if live_event is not None:
                        live_event.synchronize()
                        if int(live_host[0]) == 0:
                            break
                    live_host.copy_(cursor[1:2], non_blocking=True)
                    live_event = torch.cuda.Event(); live_event.record(stream)
                if k >= bound:
                    break
                if own_trace:                # the state every seed that has just started starts from: behind the refill, in front of the step
                    m.episode_trace_dev(S, _lib.TRACE_START, slot_seed, dx0, dobst, ep_flags=flags, ep_steps=steps, stream=s)
                m.closed_loop_step_dev(S, dx0, dobst, dgoal, X, U, u0, None, status, iters, nbuf, flags=fl,
                                       min_margin=margin, ep_flags=flags, ep_steps=steps, stream=s)
                if ft["status_log"]:
                    m.episode_status_log_dev(S, status, flags, steps, tabs["log"], stream=s)
                if own_trace:                # the step itself: the next refill overwrites a slot that has just finished
                    m.episode_trace_dev(S, _lib.TRACE_STEP, slot_seed, dx0, dobst, X, u0, status, iters, flags, steps, stream=s)
                k += 1
            stream.synchronize()
            left = int(cursor[1].item())
            ri = res_i.cpu().numpy(); rfh = res_f.cpu().numpy()
            extra = {}
            if ft["status_log"]:
                rl = tabs["res_log"].cpu().numpy()
                extra.update(status2=rl[:, 0].copy(), status4=rl[:, 1].copy(), first_bad=rl[:, 2].copy())
            if ring_cap is not None and poll_every == 1:
                extra["seed_src"] = seed_src.cpu().numpy()
            th = {n: a.cpu().numpy() for n, a in tarr.items() if a is not None and n not in ("seed_row", "slot_state")} if own_trace else None
        finally:
            stream.synchronize()
            if solver is not None:           # (a caller's solver leaves as it came; the handle holds pointers into this call's tensors)
                if own_trace:
                    m.episode_trace_set_dev(0)
                if own_tables:
                    m.set_refill_tables_dev()
                if ring_cap is not None:
                    m.episode_ring_dev(0)
                if own_params:
                    m.set_instance_params()
                if own_mask:
                    m.set_obstacle_mask(None)
                if own_bounds:
                    m.set_instance_bounds_dev(None)
                if sqp is not None:
                    m.set_sqp()
    if solver is None:
        m.close()
    if left != 0 or (ri[:, 0] < 0).any():
        raise _lib.MpcError(f"the sweep did not drain within {bound} control steps ({left} slots live, {int((ri[:, 0] < 0).sum())} rows not parked)")
    fl_h, st_h, xl = ri[:, 0], ri[:, 1], np.ascontiguousarray(rfh[:, 1:6])
    goal_all = np.ascontiguousarray(np.broadcast_to(goal, (count, 2)), dtype=np.float64)
    table = np.column_stack([(fl_h & 4) != 0, (fl_h & 1) != 0, rfh[:, 0],
                             np.linalg.norm(xl[:, :2] - goal_all, axis=1), st_h, (fl_h & 2) != 0]).astype(np.float64)
    if th is not None:
        if (th["len"] < 0).any():
            raise _lib.MpcError(f"trace: seed indices {tr['seeds'][th['len'] < 0].tolist()} started without a START launch (mpc_episode_trace_dev)")
        want = (table[tr["seeds"], 4] + table[tr["seeds"], 1]).astype(np.int64)
        if not np.array_equal(th["len"], want):
            bad = np.nonzero(th["len"] != want)[0]
            raise _lib.MpcError(f"trace: seed index {int(tr['seeds'][bad[0]])} recorded {int(th['len'][bad[0]])} control steps, its table row says {int(want[bad[0]])}")
        out = {}
        for r, ks in enumerate(tr["seeds"].tolist()):
            L = int(th["len"][r])
            out[ks] = dict(simX=th["x"][r, :L + 1].copy(), obst_traj=th["obst"][r, :L + 1].copy(), u=th["u"][r, :L].copy(), status=th["status"][r, :L].copy(),
                           iters=th["iters"][r, :L].copy())
            if tr["pred"]:
                out[ks]["pred"] = th["pred"][r, :L].copy()
        extra["trace"] = out
    return dict(table=table, x_last=xl, steps_run=k, solves=int(st_h.sum()) + int((fl_h & 1).sum()), schedule=schedule, **extra)


def sweep_record(result, k):
    """One traced seed of a sweep in run_episodes(record=True)'s layout, as a batch of one: `result` = run_seed_sweep(..., trace=...), k a traced seed index.
    Returns dict(simX (L + 1, 1, 5), obst_traj (L + 1, 1, n_obst, 4), pred (L, 1, N + 1, 5), table (1, 6), x_last (1, 5)), so that
    visualisation_inputs(sweep_record(result, k), 0) is what the reference hands to its VisDynamicRobotEnv for that seed."""
    tr = result.get("trace") if isinstance(result, dict) else None
    if tr is None:
        raise ValueError("the sweep was run without a trace: pass trace=True or the seed indices to run_seed_sweep")
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or int(k) not in tr:
        raise ValueError(f"seed index {k!r} was not traced (traced: {sorted(tr)[:8]}{' ...' if len(tr) > 8 else ''})")
    t = tr[int(k)]
    if "pred" not in t:
        raise ValueError("the trace holds no predicted horizons (trace_pred=False): a record for visualisation_inputs needs them")
    return dict(simX=t["simX"][:, None].copy(), obst_traj=t["obst_traj"][:, None].copy(), pred=t["pred"][:, None].copy(),
                table=np.array(result["table"][int(k)][None]), x_last=np.array(result["x_last"][int(k)][None]))


def visualisation_inputs(rec, instance, steps=None):
    """What the reference hands to its `VisDynamicRobotEnv` (robot_ocp_problem.py:270-276, visualization.py:135-151) for ONE instance of a
    recorded batch (`rec` = run_episodes(..., record=True)):
        trajectory   (2, T)          -> vis.set_trajectory(simX[:, :2].T)
        pred         (T, N + 1, 2)   -> vis.set_pred_trajectories(pred): row 0 zeros (init_experiment, :48-49), row k the horizon solved at step k
        obstacles    [n_obst x (2, T)] -> vis.set_obst_trajectory([o.get_trajectory().T ...])
    with T = steps + 1 (default: the instance's own episode length).  The recorded iterate is the SHIFTED one (stage j of the solve sits at
    X[j - 1], stage N is kept, :253-258) and stage 0 of a solve is the plant state it started from, so the solved horizon is re-assembled here."""
    simX, obst, pred = rec["simX"], rec["obst_traj"], rec["pred"]
    if steps is None:
        steps = int(rec["table"][instance, 4]) + int(rec["table"][instance, 1])      # control steps run: i, plus the one that reached the goal
    steps = min(steps, pred.shape[0])
    T = steps + 1
    N = pred.shape[2] - 1
    horizon = np.zeros((T, N + 1, 2))
    for k in range(steps):
        horizon[k + 1, 0] = simX[k, instance, :2]
        horizon[k + 1, 1:N] = pred[k, instance, 0:N - 1, :2]
        horizon[k + 1, N] = pred[k, instance, N, :2]
    return dict(trajectory=simX[:T, instance, :2].T.copy(), pred=horizon,
                obstacles=[obst[:T, instance, j, :2].T.copy() for j in range(obst.shape[2])])


def write_experiment(table, spec, out_dir, stamp=None):
    """experiments.py:28-43 file format: `<stamp>_experiment_data.csv` (';' separated) + `<stamp>_experiment_spec.json`."""
    os.makedirs(out_dir, exist_ok=True)
    stamp = stamp or time.strftime("%Y%m%d_%H%M%S")
    np.savetxt(os.path.join(out_dir, f"{stamp}_experiment_data.csv"), table, delimiter=";")
    with open(os.path.join(out_dir, f"{stamp}_experiment_spec.json"), "w") as f:
        json.dump(spec, f)
    return stamp
