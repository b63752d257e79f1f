"""On-device closed-loop episode harness: `RobotOcpProblem.step` + `experiments.py` semantics for a
whole batch of scenarios, one kernel launch per control step, everything resident in HBM.

Output table columns are the reference's (src/simulation/robot_ocp_problem.py:277, sliced [1:] at experiments.py:36):
    [hit, reached_goal, min_margin, dist_to_goal, iters, out_of_bounds]
and `write_experiment` stores them as `;`-separated CSV + spec JSON like experiments.py:40-43, so tooling written for the
reference's `test_data/` (evaluate_experiments.py:8-18) reads them.

Two loops carry four drivers: _episode_loop (one batch) runs run_episodes and multistart.run_multistart_episodes, _sweep_loop (seeds streaming through
slots) runs run_seed_sweep and multistart.run_multistart_sweep.  A loop holds the protocol alone -- the step counter, when the host looks at the device and
when it stops, the schedule a sweep records -- and a driver hands in its launches as callables; the loops touch no handle, so fakes on CPU tensors drive them.
Below them the drivers share _HandleLease (what a driver borrows on a handle), _sweep_table (the parked rows of either sweep) and step_flags / refill_flags /
result_table, the reference's protocol in one place each.
"""
import json
import os
import time
import warnings
from types import SimpleNamespace

import numpy as np

from . import _lib
from .solver import BOUNDS_ROW, INSTANCE_ROW, BatchedMpc, instance_rows, mask_rows, pack_instance_bounds, pack_obstacle_mask


class _HandleLease:
    """The one owner of what a driver borrows on a handle (pure Python: anything with the setters' names will do as a solver).  `solver` is a caller's
    handle or None; then the lease makes one of its own with `make()`.  Inside `with` the handle is `.m`, and every mutation of it goes through attach(),
    which registers the setter's off call as soon as the setter has returned.  On exit, normal or by exception, in this order: the driver's stream (`.stream`,
    if one was given) is synchronised -- the handle must not lose pointers a queued launch still reads, nor the tensors die before that --; the features are
    switched off in reverse order of attachment; the handle is closed if and only if the lease made it.  Off means off: a caller's earlier setting of the
    same feature is not re-created.  A step of the exit that raises does not stop the steps behind it, and the first exception (the block's own, if it
    raised) is the one that leaves."""
    OFF = {"set_instance_params": (), "set_obstacle_mask": (None,), "set_instance_bounds": (), "set_instance_bounds_dev": (None,), "set_sqp": (),
           "set_refill_tables_dev": (), "episode_ring_dev": (0,), "episode_trace_set_dev": (0,)}

    def __init__(self, solver, make, stream=None):
        self._solver, self._make, self.stream, self._attached = solver, make, stream, []

    def __enter__(self):
        self.m = self._make() if self._solver is None else self._solver
        return self

    def attach(self, setter, *args, **kw):
        """m.<setter>(*args, **kw), undone on exit by the setter's off call (a setter without one is a KeyError, and not called); the arguments -- tensors
        the handle then points into -- are kept until then"""
        off = self.OFF[setter]
        getattr(self.m, setter)(*args, **kw)
        self._attached.append((setter, off, args, kw))

    def __exit__(self, exc_type, exc, tb):
        steps = ([] if self.stream is None else [self.stream.synchronize]) + [lambda n=n, off=off: getattr(self.m, n)(*off) for n, off, _, _ in reversed(self._attached)]
        first = exc
        for step in steps + ([self.m.close] if self._solver is None else []):
            try:
                step()
            except Exception as e:
                first = e if first is None else first
        if first is not exc:
            raise first


def step_flags(init_guess_when_error=True, bug_compat_alias=True, interpolate_init=False, margin_all=False):
    """the fused control step's flag word (_lib.STEP_*) for the drivers' switches; margin_all counts only together with an obstacle mask"""
    fl = _lib.STEP_SHIFT | _lib.STEP_PLANT | _lib.STEP_OBSTACLES | _lib.STEP_METRICS | (_lib.STEP_MARGIN_ALL if margin_all else 0)
    if init_guess_when_error:
        fl |= _lib.STEP_RESET_ON_FAIL | (_lib.STEP_ALIAS_BUG if bug_compat_alias else 0) | (_lib.STEP_INTERP_GUESS if interpolate_init else 0)
    return fl


def refill_flags(bug_compat_alias=True, interpolate_init=False, random_move=True):
    """the refill's flag word (_lib.REFILL_*) for the same switches"""
    return (_lib.REFILL_ALIAS_BUG if bug_compat_alias else 0) | (_lib.REFILL_INTERP_GUESS if interpolate_init else 0) | (_lib.REFILL_DRAW_NOISE if random_move else 0)


def _warn_interpolate_alias(interpolate_init, bug_compat_alias):
    """the drivers' warning about interpolate_init together with bug_compat_alias, attributed to the driver's caller"""
    if interpolate_init and bug_compat_alias:
        warnings.warn("interpolate_init with bug_compat_alias=True: the straight-line guess is built from a plant state whose v, omega the aliasing defect has "
                      "zeroed; the two recorded `interpolate_init` tables replay with bug_compat_alias=False (tests/test_gpu_replay.py)", stacklevel=3)


def result_table(ep_flags, min_margin, x_last, goal, steps):
    """the (rows, 6) table [hit, reached, min_margin, dist_to_goal, iters, out_of_bounds] from flag words, margins, last states, goals and step counts;
    the solves behind it are table[:, 4] + table[:, 1]: every episode's control steps, plus the one that reached the goal"""
    return np.column_stack([(ep_flags & 4) != 0, (ep_flags & 1) != 0, min_margin, np.linalg.norm(x_last[:, :2] - goal, axis=1), steps, (ep_flags & 2) != 0]).astype(np.float64)


def _loop_arrays(torch, dev, rows, N, n_obst, flags0):
    """what a fused control step of `rows` instances works on beside x0, goal and obst (the driver's to fill in): iterate, status words, episode bookkeeping;
    with them the two kinds of array (.f64, .i32: keywords for torch's constructors) and the device generator's arrays, None until a driver makes them"""
    f64 = dict(dtype=torch.float64, device=dev); i32 = dict(dtype=torch.int32, device=dev)
    return SimpleNamespace(rows=rows, f64=f64, i32=i32, X=torch.zeros(rows, N + 1, 5, **f64), U=torch.zeros(rows, N, 2, **f64), status=torch.zeros(rows, **i32),
                           iters=torch.zeros(rows, **i32), margin=torch.full((rows,), float("inf"), **f64), flags=torch.full((rows,), flags0, **i32),
                           steps=torch.zeros(rows, **i32), gen_state=None, nbuf=None)


def _fused_step(m, a, fl, noise, s, u0=None):
    """one fused control step on the arrays `a`"""
    m.closed_loop_step_dev(a.rows, a.x0, a.obst, a.goal, a.X, a.U, u0, None, a.status, a.iters, noise, flags=fl, min_margin=a.margin, ep_flags=a.flags, ep_steps=a.steps, stream=s)


def _episode_noise(noise, scenario_name, seed, random_move, max_iter, B, n_obst):
    """run_episodes' `noise` and `seed`, checked on the host before anything touches a device.  Returns the source of the normals: None (the obstacles do not
    draw), "reference", "torch" or the float64 array (>= max_iter, B, n_obst, 2)."""
    if scenario_name is not None and noise is None and random_move:
        noise = "reference"
        if seed != 0:
            raise ValueError("`seed` selects torch's generator, which a scenario name does not use: the obstacle noise is the reference's own numpy stream "
                             "per instance (first_seed + s).  Vary first_seed, or pass noise='torch' to draw from torch's generator with this seed")
    noise = "torch" if noise is None else noise
    if isinstance(noise, str):
        if noise != "torch" and (noise != "reference" or scenario_name is None):
            raise ValueError("noise='reference' continues the generator of a scenario draw: pass the scenario name as `obst`")
    elif random_move:
        noise = np.ascontiguousarray(noise, dtype=np.float64)
        if noise.shape[1:] != (B, n_obst, 2) or noise.shape[0] < max_iter:
            raise ValueError(f"noise must be (>= {max_iter}, {B}, {n_obst}, 2), got {noise.shape}")
    return noise if random_move else None


def _noise_source(torch, m, a, noise, scenario_name, first_seed, seed, s):
    """run_episodes' normals as a function of the control step k, over the batch `a` as it is at that step (compaction shrinks it); allocates what the
    source needs (a.gen_state, a.nbuf: the device generator's states and its output)"""
    n_obst = a.obst.shape[1]
    if noise is None:
        return lambda k: None
    if isinstance(noise, np.ndarray):
        dnoise = torch.from_numpy(noise).to(a.obst.device)
        return lambda k: dnoise[k] if a.rows == dnoise.shape[1] else dnoise[k][a.ids]
    if noise == "torch":
        gen = torch.Generator(device=a.obst.device); gen.manual_seed(seed)
        return lambda k: torch.randn(a.rows, n_obst, 2, generator=gen, **a.f64)
    a.gen_state = m.noise_state(a.rows, scenario_name, seed0=first_seed, stream=s)
    a.nbuf = torch.zeros(a.rows, n_obst, 2, **a.f64)

    def draw(k):
        m.noise_draw_dev(a.rows, a.gen_state, a.nbuf, ep_flags=a.flags, stream=s)
        return a.nbuf
    return draw


_PARKED = ("margin", "flags", "steps", "x0")          # what compaction keeps of a finished episode


def _compact(a, full):
    """run_episodes' compaction step: once a quarter of the batch `a` has finished, the results of the finished episodes are parked in `full` under their
    ids and the live ones move together (device-side gathers).  False: no episode is live."""
    live = (a.flags & 1) == 0
    n_live = int(live.sum().item())                 # (the one host read: at these batch sizes 25 control steps take tens of milliseconds)
    if n_live == 0:
        return False
    if n_live <= 0.75 * a.rows:
        park = a.ids[~live]
        for n in _PARKED:
            full[n][park] = getattr(a, n)[~live]
        for n in ("ids", "x0", "goal", "obst", "X", "U", "status", "iters", "margin", "flags", "steps") + (("gen_state", "nbuf") if a.gen_state is not None else ()):
            setattr(a, n, getattr(a, n)[live].contiguous())
        a.rows = n_live
    return True


def _episode_loop(torch, stream, max_iter, step, flags, every_25=None):
    """The batch drivers' control steps: step(k) -- the driver's launches of control step k -- until every episode has reached its goal or max_iter steps are
    spent.  flags(): the episodes' flag words as they stand (compaction rebinds them).  every_25(k), if given, stands in for the done-flag copy behind every
    25th step (run_episodes' compaction, which reads the live count anyway); False: no episode is live.  Returns the steps launched."""
    # "every instance has reached its goal" without stalling the queue: every 25 control steps the flag goes to pinned host memory behind an event,
    # and is looked at only once that event has passed (so the loop runs at most ~25 steps longer than it has to -- on idle instances, which cost nothing)
    done_host = done_event = None
    k = 0
    while k < max_iter:
        step(k)
        k += 1
        if done_event is not None and done_event.query():
            if int(done_host[0]) == 1:
                break
            done_event = None
        if k % 25 != 0:
            continue
        if every_25 is not None:
            if not every_25(k):
                break
        elif done_event is None:
            if done_host is None:      # (the first poll: a loop that ends before it needs no pinned memory)
                done_host = torch.zeros(1, dtype=torch.int32).pin_memory()
            done_host.copy_((flags() & 1).min().to(torch.int32).reshape(1), non_blocking=True)
            done_event = torch.cuda.Event(); done_event.record(stream)
    return k


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
    solver: a caller's handle to run on.  It leaves as it came whether the call returns or raises (_HandleLease): radii, mask, bounds and SQP setting of this
    call are switched OFF again -- a setting of the same feature the caller had made before is not re-created.  The arguments that need no device (noise, seed)
    are checked before the handle is touched.
    Returns dict(table (B,6), x_last (B,5), steps_run, solves)."""
    x0 = np.ascontiguousarray(x0, dtype=np.float64); B = x0.shape[0]
    scenario_name = obst if isinstance(obst, str) else None
    if scenario_name is None:
        obst = np.ascontiguousarray(obst, dtype=np.float64); n_obst = obst.shape[1]
    _warn_interpolate_alias(interpolate_init, bug_compat_alias)
    noise = _episode_noise(noise, scenario_name, seed, random_move, max_iter, B, n_obst)
    import torch
    if scenario_name is not None:
        with BatchedMpc(N, n_obst, Tf, max_batch=B, device=device) as g:
            obst = np.ascontiguousarray(g.generate_scenarios(scenario_name, B, seed0=first_seed), dtype=np.float64)
    goal = np.ascontiguousarray(np.broadcast_to(goal, (B, 2)), dtype=np.float64)
    dev = torch.device("cuda", device)
    with _HandleLease(solver, lambda: BatchedMpc(N, n_obst, Tf, max_batch=B, device=device, **cfg)) as lease:
        m = lease.m
        own_features = False            # radii, mask or bounds per episode: such a batch is not compacted
        if r_safe is not None or r_hit is not None:
            lease.attach("set_instance_params", r_safe=r_safe, r_hit=r_hit); own_features = True
        if active is not None:
            lease.attach("set_obstacle_mask", np.asarray(active)); own_features = True
        if bounds is not None:
            lease.attach("set_instance_bounds", **bounds); own_features = True
        if sqp is not None:
            lease.attach("set_sqp", *sqp)
        lease.stream = stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(stream):
            t = lambda h: torch.from_numpy(h.copy()).to(dev)
            a = _loop_arrays(torch, dev, B, N, n_obst, 0)
            a.x0, a.goal, a.obst = t(x0), t(goal), t(obst)
            if bug_compat_alias:                      # set_initial_guess() aliases self.x0 and zeroes v, omega (defect D2)
                a.x0[:, 3:] = 0.0
            s = stream.cuda_stream
            if interpolate_init:
                m.reset_guess_interp_dev(B, a.x0, a.goal, a.X, a.U, stream=s)
            else:
                m.reset_guess_dev(B, a.x0, a.X, a.U, stream=s)        # set_initial_guess() at the start of step(), :180
            fl = step_flags(init_guess_when_error, bug_compat_alias, interpolate_init, margin_all and active is not None)
            log = SimpleNamespace(n2=torch.zeros(B, **a.i32), n4=torch.zeros(B, **a.i32), first_bad=torch.full((B,), -1, **a.i32)) if status_log else None
            draw = _noise_source(torch, m, a, noise, scenario_name, first_seed, seed, s)
            # compaction of finished episodes (compact_from): results of parked episodes live in full-size arrays, `ids` maps the live batch to them
            full = None
            if compact_from is not None and B >= compact_from and not record and not status_log and not own_features:
                a.ids = torch.arange(B, device=dev)
                full = {n: getattr(a, n).clone() for n in _PARKED}
            rec = SimpleNamespace(x=[a.x0.clone()], o=[a.obst.clone()], p=[]) if record else None
            def step(k):
                _fused_step(m, a, fl, draw(k), s)
                if log is not None:      # (an episode that has reached its goal idles: its status word keeps the last solve's value and is not counted again)
                    live = (a.steps + (a.flags & 1)) > k
                    log.n2 += (live & (a.status == 2)).int(); log.n4 += (live & (a.status == 4)).int()
                    log.first_bad = torch.where(live & (a.status != 0) & (log.first_bad < 0), torch.full_like(log.first_bad, k), log.first_bad)
                if rec is not None:      # X holds the shifted prediction: stage j of the solve is X[j - 1], stage N is kept (:253-258)
                    rec.x.append(a.x0.clone()); rec.o.append(a.obst.clone()); rec.p.append(a.X.clone())
            k = _episode_loop(torch, stream, max_iter, step, lambda: a.flags, every_25=None if full is None else lambda k: _compact(a, full))
            stream.synchronize()
            if full is not None:
                for n in _PARKED:
                    full[n][a.ids] = getattr(a, n)
                a = SimpleNamespace(**full)
            fl_h = a.flags.cpu().numpy(); xl = a.x0.cpu().numpy()
            table = result_table(fl_h, a.margin.cpu().numpy(), xl, goal, a.steps.cpu().numpy())
            extra = dict(simX=torch.stack(rec.x).cpu().numpy(), obst_traj=torch.stack(rec.o).cpu().numpy(), pred=torch.stack(rec.p).cpu().numpy()) if record else {}
            if status_log:
                extra.update(status2=log.n2.cpu().numpy(), status4=log.n4.cpu().numpy(), first_bad=log.first_bad.cpu().numpy())
    return dict(table=table, x_last=xl, steps_run=k, solves=int(table[:, 4].sum() + table[:, 1].sum()), **extra)


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
            _seed_rows(name, a, count)
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


def _seed_rows(name, a, count):
    """a per-seed array `a` holds one row per seed"""
    if a.shape[0] != count:
        raise ValueError(f"per-seed {name} has {a.shape[0]} rows for {count} seeds")
    return a


def _sweep_features(count, n_obst, handle_cfg, r_safe=None, r_hit=None, W=None, We=None, active=None, margin_all=False, bounds=None, status_log=False,
                    ring=None, ring_every=None, poll_every=25):
    """run_seed_sweep's per-seed arguments, checked on the host before anything touches a device: shapes by the setters' own rules (solver.instance_rows,
    mask_rows, pack_instance_bounds), values here, because the tables go to the _dev setters, which validate nothing.  handle_cfg: an object with the
    handle's bx_lo, bx_hi, bu_lo, bu_hi (an MpcConfig, or a dict over DEFAULT_BOUNDS).  Returns dict(W, We, r_safe, r_hit (float64 (count, .) or None),
    mask (int32 words (count,) or None), bounds (float64 (count, 12) or None), margin_all, status_log, ring (capacity or None), ring_every)."""
    out = dict(margin_all=bool(margin_all), status_log=bool(status_log))
    for (name, cols), a in zip(INSTANCE_ROW, (W, We, r_safe, r_hit)):
        if a is not None:
            a = _seed_rows(name, instance_rows(name, a, cols, n_obst, rows="count"), count)
            if not np.isfinite(a).all() or not ((a > 0.0) if cols is None else (a >= 0.0)).all():          # (cols None: a radius)
                raise ValueError(f"per-seed {name} must be finite and " + ("> 0" if cols is None else ">= 0"))
        out[name] = a
    out["mask"] = None
    if active is not None:
        a = _seed_rows("active", mask_rows(active, n_obst, rows="count", why=": a mask has no bit at or above n_obst"), count)
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
            if v.ndim == 2:
                _seed_rows(n, v, count)
            if not np.isfinite(v).all():
                raise ValueError(f"bounds: {n} entries must be finite")
        get = (lambda n: handle_cfg[n]) if isinstance(handle_cfg, dict) else (lambda n: list(getattr(handle_cfg, n)))
        own = type("Cfg", (), {n: get(n) for n, _, _ in BOUNDS_ROW})
        tab = pack_instance_bounds(own, count, rows="count", **given)
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


def _sweep_slots(torch, dev, m, S, count, start, goal, random_move):
    """the sweep's device state: the start and goal rows, the per-slot arrays of mpc_episode_refill_dev for S slots, its cursor and the result rows of
    `count` seeds"""
    a = _loop_arrays(torch, dev, S, m.N, m.n_obst, 1)          # every slot "finished" and without a seed: the first refill fills them all
    a.count = count
    a.start_rows, a.goal_rows = torch.from_numpy(start).to(dev), torch.from_numpy(goal).to(dev)
    a.x0 = torch.zeros(S, 5, **a.f64); a.goal = torch.zeros(S, 2, **a.f64); a.obst = torch.zeros(S, m.n_obst, 4, **a.f64)
    a.slot_seed = torch.full((S,), -1, **a.i32); a.cursor = torch.zeros(2, **a.i32)
    a.gen_state = torch.zeros(S, _lib.lib().mpc_noise_state_words(), **a.i32)
    a.nbuf = torch.zeros(S, m.n_obst, 2, **a.f64) if random_move else None
    a.res_f = torch.full((count, 6), float("nan"), **a.f64); a.res_i = torch.full((count, 2), -1, **a.i32)
    return a


def _attach_tables(lease, torch, a, ft):
    """per-seed tables: the sources (count rows) and the per-slot arrays the solve reads in place (max_batch rows, preset with the handle's own values: a
    slot that never gets a seed holds valid numbers), registered with the _dev setters; the refill copies row k into the slot that starts k.  With them the
    status log's per-slot words and result rows.  Returns the tensors by their names in set_refill_tables_dev ({}: nothing to attach)."""
    m, dev = lease.m, a.x0.device
    MB, n_obst = m.max_batch, m.n_obst
    tabs = {}
    if any(ft[n] is not None for n, _ in INSTANCE_ROW):
        r_hit_own = 1.0 + 0.2                               # o.r + R_ROBOT: the fused step's hit radius (mpc_closed_loop_step_dev)
        preset = dict(W=list(m.cfg.W), We=list(m.cfg.We), r_safe=[m.cfg.r_safe] * n_obst, r_hit=[r_hit_own] * n_obst)
        slot = {}
        for name, _ in INSTANCE_ROW:
            if ft[name] is not None:
                tabs[name] = torch.from_numpy(ft[name]).to(dev)
                slot[name] = tabs["slot_" + name] = torch.tensor(preset[name], **a.f64).repeat(MB, 1).contiguous()
        lease.attach("set_instance_params", **slot)
    if ft["mask"] is not None:
        tabs["mask"] = torch.from_numpy(ft["mask"].copy()).to(dev)
        tabs["slot_mask"] = torch.full((MB,), int(np.array([(1 << n_obst) - 1], dtype=np.uint32).view(np.int32)[0]), **a.i32)
        lease.attach("set_obstacle_mask", tabs["slot_mask"])
    if ft["bounds"] is not None:
        tabs["bounds"] = torch.from_numpy(ft["bounds"]).to(dev)
        tabs["slot_bounds"] = torch.from_numpy(pack_instance_bounds(m.cfg, MB)).to(dev)
        lease.attach("set_instance_bounds_dev", tabs["slot_bounds"])
    if ft["status_log"]:
        tabs["log"] = torch.tensor([0, 0, -1, 0], **a.i32).repeat(a.rows, 1).contiguous()
        tabs["res_log"] = torch.full((a.count, 3), -1, **a.i32)
    if tabs:
        lease.attach("set_refill_tables_dev", **tabs)
    return tabs


def _attach_ring(lease, torch, a, capacity):
    """the ring of seeded episodes (mpc_episode_ring_dev) for the slots `a`.  Returns its tensors: dict(ring_state, ring_obst, ring_tag, seed_src)"""
    ring = dict(ring_state=torch.zeros(capacity, a.gen_state.shape[1], **a.i32), ring_obst=torch.zeros(capacity, lease.m.n_obst, 4, **a.f64),
                ring_tag=torch.full((capacity,), -1, **a.i32), seed_src=torch.full((a.count,), -1, **a.i32))
    lease.attach("episode_ring_dev", capacity, **ring)
    return ring


def _attach_trace(lease, torch, a, tr, max_iter):
    """the per-seed rows (mpc_episode_trace) for the slots `a`: row r belongs to seed index tr["seeds"][r].  Returns (the arrays by their names in
    episode_trace_set_dev, the u* array (slots, 2) the fused step then writes)"""
    R, N, n_obst, f64, i32 = tr["seeds"].size, lease.m.N, lease.m.n_obst, a.f64, a.i32
    tarr = dict(seed_row=torch.from_numpy(tr["seed_row"]).to(a.x0.device), slot_state=torch.tensor([-1, 0], **i32).repeat(a.rows, 1).contiguous(),
                len=torch.zeros(R, **i32), x=torch.zeros(R, max_iter + 1, 5, **f64), obst=torch.zeros(R, max_iter + 1, n_obst, 4, **f64),
                u=torch.zeros(R, max_iter, 2, **f64), status=torch.zeros(R, max_iter, **i32), iters=torch.zeros(R, max_iter, **i32),
                pred=torch.zeros(R, max_iter, N + 1, 5, **f64) if tr["pred"] else None)
    u0 = torch.zeros(a.rows, 2, **f64)
    lease.attach("episode_trace_set_dev", R, max_iter, **tarr)
    return tarr, u0


def _sweep_loop(torch, stream, rows, count, slot_seed, cursor, poll_every, bound, refill, step):
    """The sweep drivers' control steps, each one: refill(k) -- the driver's launches that park finished rows and start seeds, which leave the seed index of
    every one of the `rows` slots (or groups) in slot_seed and the live count in cursor[1] --, the poll, the bound check, step(k) -- the driver's launches of
    control step k -- until the poll sees no live row, or `bound` steps are spent whatever the device returns.
    Returns (the steps launched, the schedule (count, 2) with poll_every = 1 or None)."""
    schedule = np.full((count, 2), -1, dtype=np.int64) if poll_every == 1 else None
    seen = np.full(rows, -1, dtype=np.int64)
    live_host = live_event = None
    k = 0
    while True:
        refill(k)
        if poll_every == 1:
            now = slot_seed.cpu().numpy()              # (blocking: this is the mode that records the schedule, not the one that is timed)
            new = (now != seen) & (now >= 0)
            schedule[now[new], 0] = np.nonzero(new)[0]; schedule[now[new], 1] = k
            seen[:] = now                              # (by value: a host tensor's .cpu() is the tensor itself)
            if int(cursor[1].item()) == 0:
                break
        elif k % poll_every == 0:
            # the count of the poll before this one, which the device passed long ago: the host stays at most two polls ahead of the device (no idle
            # steps by the hundred behind the end of the sweep) and the device always has a poll's worth of steps queued (it never waits for the host)
            if live_event is not None:
                live_event.synchronize()
                if int(live_host[0]) == 0:
                    break
            else:                                      # (the first poll of the event mode: the blocking mode needs no pinned memory)
                live_host = torch.full((1,), -1, dtype=torch.int32).pin_memory()
            live_host.copy_(cursor[1:2], non_blocking=True)
            live_event = torch.cuda.Event(); live_event.record(stream)
        if k >= bound:
            break
        step(k)
        k += 1
    return k, schedule


def _sweep_table(cursor, res_i, res_f, goal, bound, noun):
    """the parked rows of either sweep on the host, once its stream has drained: cursor[1] = the live count, res_f[k] = seed index k's min_margin and last state,
    res_i[k] = its flag word, its step count and what the driver parks behind them (-1: not parked); noun: the driver's rows ("slots" | "groups").
    Returns (table (count, 6), x_last (count, 5), the raw res_i) -- or MpcError: the sweep has not drained."""
    left = int(cursor[1].item())
    ri = res_i.cpu().numpy(); rfh = res_f.cpu().numpy()
    if left != 0 or (ri[:, 0] < 0).any():
        raise _lib.MpcError(f"the sweep did not drain within {bound} control steps ({left} {noun} live, {int((ri[:, 0] < 0).sum())} rows not parked)")
    xl = np.ascontiguousarray(rfh[:, 1:6])
    return result_table(ri[:, 0], rfh[:, 0], xl, np.ascontiguousarray(np.broadcast_to(goal, (ri.shape[0], 2)), dtype=np.float64), ri[:, 1]), xl, ri


def _sweep_collect(a, goal, bound, tabs, seed_src, tarr, tr):
    """the sweep's results on the host, once its stream has drained: table and x_last from the parked rows, the status log, seed_src (None: not recorded),
    the traced rows cut to each seed's length -- held to the table's lengths.  Returns the result dict without steps_run and schedule."""
    table, xl, _ = _sweep_table(a.cursor, a.res_i, a.res_f, goal, bound, "slots")
    out = dict(table=table, x_last=xl, solves=int(table[:, 4].sum() + table[:, 1].sum()))
    if "res_log" in tabs:
        rl = tabs["res_log"].cpu().numpy()
        out.update(status2=rl[:, 0].copy(), status4=rl[:, 1].copy(), first_bad=rl[:, 2].copy())
    if seed_src is not None:
        out["seed_src"] = seed_src.cpu().numpy()
    if tarr is not None:
        th = {n: t.cpu().numpy() for n, t in tarr.items() if t is not None and n not in ("seed_row", "slot_state")}
        if (th["len"] < 0).any():
            raise _lib.MpcError(f"trace: seed indices {tr['seeds'][th['len'] < 0].tolist()} started without a START launch (mpc_episode_trace_dev)")
        want = (table[tr["seeds"], 4] + table[tr["seeds"], 1]).astype(np.int64)
        if not np.array_equal(th["len"], want):
            bad = np.nonzero(th["len"] != want)[0]
            raise _lib.MpcError(f"trace: seed index {int(tr['seeds'][bad[0]])} recorded {int(th['len'][bad[0]])} control steps, its table row says {int(want[bad[0]])}")
        cut = dict(simX=("x", 1), obst_traj=("obst", 1), u=("u", 0), status=("status", 0), iters=("iters", 0), pred=("pred", 0))      # (array, rows beyond L)
        out["trace"] = {ks: {n: th[src][r, :int(th["len"][r]) + more].copy() for n, (src, more) in cut.items() if src in th} for r, ks in enumerate(tr["seeds"].tolist())}
    return out


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
    solver: a caller's handle (max_batch >= the slots) to run on.  It leaves as it came whether the call returns or raises (_HandleLease): SQP setting, per-seed
    tables, ring and trace of this call are switched OFF again, and the handle keeps no pointer into this call's tensors -- a setting of the same feature the
    caller had made before is not re-created.
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
    _warn_interpolate_alias(interpolate_init, bug_compat_alias)
    import torch
    S = min(int(slots), count); max_iter = int(max_iter); poll_every = int(poll_every)
    bound = -(-count // S) * max_iter + poll_every
    fl = step_flags(init_guess_when_error, bug_compat_alias, interpolate_init, ft["margin_all"] and ft["mask"] is not None)
    rf = refill_flags(bug_compat_alias, interpolate_init, random_move)
    dev = torch.device("cuda", device)
    with _HandleLease(solver, lambda: BatchedMpc(N, n_obst, Tf, max_batch=S, device=device, **cfg)) as lease:
        m = lease.m
        if sqp is not None:
            lease.attach("set_sqp", *sqp)
        lease.stream = stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(stream):
            a = _sweep_slots(torch, dev, m, S, count, start, goal, random_move)
            tabs = _attach_tables(lease, torch, a, ft)
            ring = _attach_ring(lease, torch, a, ft["ring"]) if ft["ring"] is not None else None
            tarr, u0 = _attach_trace(lease, torch, a, tr, max_iter) if tr is not None else (None, None)
            s, log, ring_every = stream.cuda_stream, tabs.get("log"), ft["ring_every"] if ring is not None else None
            def refill(k):
                if ring_every is not None and k % ring_every == 0:
                    m.episode_ring_fill_dev(scenario, first, count, a.cursor, stream=s)
                m.episode_refill_dev(S, scenario, first, count, max_iter, a.start_rows, a.goal_rows, per_seed, a.x0, a.obst, a.goal, a.X, a.U, a.margin, a.flags,
                                     a.steps, a.gen_state, a.nbuf, a.slot_seed, a.cursor, a.res_f, a.res_i, flags=rf, stream=s)
            def step(k):
                if u0 is not None:           # the state every seed that has just started starts from: behind the refill, in front of the step
                    m.episode_trace_dev(S, _lib.TRACE_START, a.slot_seed, a.x0, a.obst, ep_flags=a.flags, ep_steps=a.steps, stream=s)
                _fused_step(m, a, fl, a.nbuf, s, u0=u0)
                if log is not None:
                    m.episode_status_log_dev(S, a.status, a.flags, a.steps, log, stream=s)
                if u0 is not None:           # the step itself: the next refill overwrites a slot that has just finished
                    m.episode_trace_dev(S, _lib.TRACE_STEP, a.slot_seed, a.x0, a.obst, a.X, u0, a.status, a.iters, a.flags, a.steps, stream=s)
            k, schedule = _sweep_loop(torch, stream, S, count, a.slot_seed, a.cursor, poll_every, bound, refill, step)
            stream.synchronize()
            out = _sweep_collect(a, goal, bound, tabs, ring["seed_src"] if ring is not None and poll_every == 1 else None, tarr, tr)
    return dict(out, steps_run=k, schedule=schedule)


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
