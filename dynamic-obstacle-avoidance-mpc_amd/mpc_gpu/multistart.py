"""MultiStartMpc: K initial guesses per scenario, the best kept on the device (include/mpc_gpu.h, MULTI-START).

The problem is non-convex: an obstacle on the line from robot to goal splits the solutions into "pass left" and "pass right", and an RTI / SQP iteration
stays in the family its guess sits in.  A MultiStartMpc of `scenarios` groups sits over ONE BatchedMpc of scenarios * K instances -- member k of group g is
instance g K + k, and every member of a group is given the group's x0, obstacles and goal -- and runs, per solve, three launches on one stream:

    mpc_seed_guesses_dev  ->  the ordinary solve launch (closed_loop_step_dev with flags = 0: the look-ahead fused)  ->  mpc_select_best_dev (broadcast)

select_by="rollout" puts two launches between the solve and the selection -- mpc_predict_dev on the G scenario rows and mpc_rollout_merit_dev on the members'
solved (X, U) with members = K -- and the selection then compares the candidates' ROLLOUT MERITS, the NLP objective of what the plant does under each U,
instead of the costs the solve reports for iterates that need not be dynamically consistent.

Nothing leaves the device between them: torch replicates the group inputs and carries the tensors, the `_dev` entry points do the work.  The pure helpers
(`check_offsets`, `check_guess_geometry`, `check_margin`, `check_select_by`, `check_group_shapes`, `replicate`, `episode_arguments`) import without a GPU.

The CLOSED LOOP has two forms.  step() composes a control step from the entry points above and the plant / obstacle / shift / seed launches.  step_fused()
runs the member solve and then ONE launch, mpc_group_step_dev (select, plant, obstacles, episode bookkeeping per group, next iterates, the members' inputs;
DESIGN.md section 4m), and run_multistart_episodes drives it to the reference's result table.  run_multistart_sweep streams more seeds than there are
groups through the groups: a finished group starts the next seed on the device (mpc_group_refill_dev).  Neither driver has a loop of
its own: they hand their launches to episodes._episode_loop and episodes._sweep_loop, the two loops run_episodes and run_seed_sweep run on, and the sweep's
rows come back through episodes._sweep_table.  PipelinedMpc does not know about groups.  run_multistart_episodes(record=...) returns the
closed-loop record of the groups that ask for it -- trajectory, applied inputs and, per step, the K candidates with the winner -- written on the device around
the group tail (mpc_group_record_dev); multistart_record hands one group to episodes.visualisation_inputs.

guess_geometry (off by default) replaces the fixed lateral offsets of members 1 .. K - 1 by amplitudes computed on the device from the obstacles that are in the
way -- the pass-left / pass-right candidates of the nearest blocking obstacles (mpc_set_guess_geometry); `offsets` is then the base family a
member falls back to."""
import numpy as np

from . import _lib
from .solver import BatchedMpc

DEFAULT_OFFSETS = (0.0, 2.5, -2.5, 5.0, -5.0)      # lateral offsets in metres; member 0 is the straight line
MAX_MEMBERS = 64                                   # one member per lane of the group's wavefront (mpc_select_best_dev)


def check_offsets(offsets):
    """the lateral offsets of a group as a float64 array (K,), 1 <= K <= 64, every entry finite -- or ValueError"""
    a = np.asarray(offsets, dtype=np.float64)
    if a.ndim != 1 or not 1 <= a.shape[0] <= MAX_MEMBERS:
        raise ValueError(f"offsets must be a sequence of 1 .. {MAX_MEMBERS} lateral offsets (one per member of a group), got shape {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError("offsets must be finite")
    return np.ascontiguousarray(a)


def check_margin(incumbent_margin):
    """the hysteresis margin of mpc_select_best_dev as a float in [0, 1) -- or ValueError (NaN included)"""
    m = float(incumbent_margin)
    if not (0.0 <= m < 1.0):
        raise ValueError(f"incumbent_margin must be in [0, 1), got {incumbent_margin}")
    return m


GUESS_GEOMETRY_DEFAULTS = dict(clearance=0.25, a_max=6.0, lead=0.0)      # metres beside r_safe, the largest amplitude in metres, seconds the obstacle is moved ahead


def check_guess_geometry(guess_geometry):
    """the guess-geometry setting of a MultiStartMpc: None or False (off) -> None; True -> the defaults; a dict with some of clearance >= 0, a_max > 0, lead >= 0
    (finite floats) -> the defaults with those entries -- or ValueError"""
    if guess_geometry is None or guess_geometry is False:
        return None
    if guess_geometry is True:
        return dict(GUESS_GEOMETRY_DEFAULTS)
    if not isinstance(guess_geometry, dict):
        raise ValueError(f"guess_geometry must be None, True or a dict with some of {sorted(GUESS_GEOMETRY_DEFAULTS)}, got {guess_geometry!r}")
    unknown = sorted(set(guess_geometry) - set(GUESS_GEOMETRY_DEFAULTS))
    if unknown:
        raise ValueError(f"guess_geometry has no entry {unknown[0]!r}: the entries are {sorted(GUESS_GEOMETRY_DEFAULTS)}")
    out = dict(GUESS_GEOMETRY_DEFAULTS)
    for k, v in guess_geometry.items():
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"guess_geometry[{k!r}] must be a number, got {v!r}")
        out[k] = float(v)
    for k in ("clearance", "lead"):
        if not (0.0 <= out[k] < np.inf):
            raise ValueError(f"guess_geometry[{k!r}] must be finite and >= 0, got {out[k]}")
    if not (0.0 < out["a_max"] < np.inf):
        raise ValueError(f"guess_geometry['a_max'] must be finite and > 0, got {out['a_max']}")
    return out


SELECT_BY = ("cost", "rollout")


def check_select_by(select_by):
    """what the selection compares: "cost" (the cost the solve reports) or "rollout" (mpc_rollout_merit_dev's merit) -- or ValueError"""
    if not isinstance(select_by, str) or select_by not in SELECT_BY:
        raise ValueError(f"select_by must be one of {SELECT_BY}, got {select_by!r}")
    return select_by


def check_group_shapes(scenarios, n_obst, x0, obstacles, goal):
    """the shapes of one group solve's inputs: x0 (G, 5), obstacles (G, n_obst, 4), goal (G, 2) with G = scenarios -- or ValueError.  Works on anything
    with a .shape (numpy arrays, torch tensors); values are not looked at."""
    G = int(scenarios)
    for name, a, want in (("x0", x0, (G, 5)), ("obstacles", obstacles, (G, int(n_obst), 4)), ("goal", goal, (G, 2))):
        if tuple(a.shape) != want:
            raise ValueError(f"{name} must be {want} (one row per scenario), got {tuple(a.shape)}")


def check_scenarios(scenarios, K):
    G = int(scenarios)
    if G < 1:
        raise ValueError(f"scenarios must be >= 1, got {scenarios}")
    if not 1 <= int(K) <= MAX_MEMBERS:
        raise ValueError(f"K must be in 1 .. {MAX_MEMBERS}, got {K}")
    return G


def replicate(a, K):
    """a per-scenario numpy array (G, ...) -> the per-instance array (G K, ...) of the group layout: row g K + k = row g"""
    a = np.asarray(a)
    return np.ascontiguousarray(np.repeat(a, int(K), axis=0))


class MultiStartMpc:
    """`scenarios` groups of K = len(offsets) candidate iterates over one BatchedMpc(N, n_obst, Tf, max_batch=scenarios * K, **cfg) (`.inner`).
    Inputs and outputs are float64 / int32 device tensors; a numpy array is uploaded.  Everything runs on the object's own stream, which waits for the
    caller's current torch stream on entry and which that stream waits for on exit."""

    def __init__(self, N=20, n_obst=3, Tf=2.0, scenarios=1, offsets=DEFAULT_OFFSETS, incumbent_margin=0.0, device=0, select_by="cost", guess_geometry=None, **cfg):
        self.select_by = check_select_by(select_by)
        self.guess_geometry = check_guess_geometry(guess_geometry)
        import torch
        off = check_offsets(offsets)
        self.K, self.G = int(off.shape[0]), check_scenarios(scenarios, off.shape[0])
        self.margin = check_margin(incumbent_margin)
        self.B = self.G * self.K
        self.inner = BatchedMpc(N, n_obst, Tf, max_batch=self.B, device=device, **cfg)
        self.N, self.n_obst = self.inner.N, self.inner.n_obst
        self._torch, self.dev = torch, torch.device("cuda", int(device))
        self.stream = torch.cuda.Stream(device=self.dev)
        G, K, B, N, no = self.G, self.K, self.B, self.N, self.n_obst
        f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=self.dev)
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=self.dev)
        self.offsets, self.offsets_host = torch.from_numpy(off).to(self.dev), off
        self.X, self.U = f64(B, N + 1, 5), f64(B, N, 2)                      # the iterates of all members
        self._x0, self._obst, self._goal = f64(G, K, 5), f64(G, K, no, 4), f64(G, K, 2)      # the group inputs, replicated per member
        self.cand_u0, self.cand_cost, self.cand_status, self.cand_iters = f64(B, 2), f64(B), i32(B), i32(B)
        self.winner, self.cost, self.u0 = i32(G), f64(G), f64(G, 2)
        self._xn, self._X1, self._U1 = f64(G, 5), f64(G, N + 1, 5), f64(G, N, 2)      # plant output; the reseed of member 0 of a failed group
        if self.select_by == "rollout":      # the scenarios' look-ahead (one row per group) and what the rollout reports per candidate
            self._P = f64(G, N + 1, no, 2)
            self.cand_merit, self.cand_defect, self.cand_margin = f64(B), f64(B), f64(B)
        self.solved_X = self.solved_U = None
        self._warm = self._fused_warm = False
        self._recording = False                    # a per-group record is attached (group_record_set_dev): step_fused launches its two phases
        self.member_offsets = None                 # guess_geometry: the (G, K) amplitudes the last stand-alone seed launch wrote
        if self.guess_geometry is not None:
            q = self.guess_geometry
            _lib.check(_lib.lib().mpc_set_guess_geometry(self.inner._h, 1, q["clearance"], q["a_max"], q["lead"]))
            self.member_offsets = f64(G, K)
        torch.cuda.synchronize(self.dev)

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "inner", None) is not None:
            self.stream.synchronize()
            self.inner.close()
            self.inner = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------ pass-through to the inner handle, replicated per group
    def set_sqp(self, max_iter=1, step_tol=0.0):
        """several SQP iterations per solve launch for every member (BatchedMpc.set_sqp)"""
        self.inner.set_sqp(max_iter, step_tol)

    def set_instance_params(self, W=None, We=None, r_safe=None, r_hit=None):
        """per-SCENARIO cost weights and radii, numpy arrays of G rows (BatchedMpc.set_instance_params), every member of a group getting its group's row"""
        rep = [None if a is None else replicate(self._rows(n, a), self.K) for n, a in (("W", W), ("We", We), ("r_safe", r_safe), ("r_hit", r_hit))]
        self.inner.set_instance_params(*rep)

    def set_obstacle_mask(self, active=None):
        """per-SCENARIO obstacle masks, a bool array (G, n_obst) (BatchedMpc.set_obstacle_mask); None switches off"""
        self.inner.set_obstacle_mask(None if active is None else replicate(self._rows("active", active), self.K))

    def set_instance_bounds(self, bx_lo=None, bx_hi=None, bu_lo=None, bu_hi=None):
        """per-SCENARIO box bounds, numpy arrays of G rows or one row for all (BatchedMpc.set_instance_bounds)"""
        rep = lambda n, a: None if a is None else (np.asarray(a, dtype=np.float64) if np.asarray(a).ndim == 1 else replicate(self._rows(n, a), self.K))
        self.inner.set_instance_bounds(rep("bx_lo", bx_lo), rep("bx_hi", bx_hi), rep("bu_lo", bu_lo), rep("bu_hi", bu_hi))

    def _rows(self, name, a):
        a = np.asarray(a)
        if a.ndim < 1 or a.shape[0] != self.G:
            raise ValueError(f"{name} must have one row per scenario ({self.G}), got shape {a.shape}")
        return a

    # ------------------------------------------------------------------ the group solve
    def _dev(self, a):
        torch = self._torch
        if isinstance(a, torch.Tensor):
            return a.to(device=self.dev, dtype=torch.float64)
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)

    def _load(self, x0, obstacles, goal):
        """the group inputs into the replicated per-member tensors (torch broadcasts the member axis)"""
        check_group_shapes(self.G, self.n_obst, x0, obstacles, goal)
        self._x0.copy_(self._dev(x0)[:, None, :])
        self._obst.copy_(self._dev(obstacles)[:, None, :, :])
        self._goal.copy_(self._dev(goal)[:, None, :])

    def _seed(self, x_rows, goal_rows, keep_first, s, obst_rows=None):
        """mpc_seed_guesses_dev from per-GROUP rows: x_rows (G, 5) and goal_rows (G, 2), contiguous; with guess_geometry mpc_seed_guesses_geom_dev on them and
        obst_rows (G, n_obst, 4), the amplitudes into member_offsets"""
        if self.guess_geometry is not None:
            _lib.check(_lib.lib().mpc_seed_guesses_geom_dev(self.inner._h, self.G, self.K, x_rows.data_ptr(), obst_rows.data_ptr(), goal_rows.data_ptr(),
                                                            self.offsets.data_ptr(), 1 if keep_first else 0, self.X.data_ptr(), self.U.data_ptr(),
                                                            self.member_offsets.data_ptr(), s))
            return
        _lib.check(_lib.lib().mpc_seed_guesses_dev(self.inner._h, self.G, self.K, x_rows.data_ptr(), goal_rows.data_ptr(), self.offsets.data_ptr(),
                                                   1 if keep_first else 0, self.X.data_ptr(), self.U.data_ptr(), s))

    def _select_key(self, x, obst, goal, s):
        """what the selection compares, behind the member solve: the costs it reports, or (select_by="rollout") the merits of predict_dev on the G group rows
        `obst` and rollout_merit_dev on the members' (X, U) from the group rows x and goal.  The rows are made contiguous only where they are read (the
        member-0 views of the replicated inputs are not; a caller's tensors are, and are passed as they are)."""
        if self.select_by != "rollout":
            return self.cand_cost
        self.inner.predict_dev(self.G, obst.contiguous(), self._P, stream=s)
        self.inner.rollout_merit_dev(self.B, x.contiguous(), self._P, goal.contiguous(), self.U, X=self.X, merit=self.cand_merit, defect=self.cand_defect,
                                     margin=self.cand_margin, members=self.K, stream=s)
        return self.cand_merit

    def _solve(self, x0, obstacles, goal, seed, keep_first, keep_solution, s):
        self._load(x0, obstacles, goal)
        if seed:
            self._seed(self._x0[:, 0].contiguous(), self._goal[:, 0].contiguous(), keep_first, s, self._obst[:, 0].contiguous())
        self.inner.closed_loop_step_dev(self.B, self._x0, self._obst, self._goal, self.X, self.U, self.cand_u0, self.cand_cost, self.cand_status,
                                        self.cand_iters, flags=0, stream=s)
        if keep_solution:
            self.solved_X, self.solved_U = self.X.clone(), self.U.clone()
        by = self._select_key(self._x0[:, 0], self._obst[:, 0], self._goal[:, 0], s)
        _lib.check(_lib.lib().mpc_select_best_dev(self.inner._h, self.G, self.K, by.data_ptr(), self.cand_status.data_ptr(), self.margin,
                                                  _lib.SELECT_BROADCAST, self.X.data_ptr(), self.U.data_ptr(), self.winner.data_ptr(),
                                                  self.cost.data_ptr(), self.u0.data_ptr(), self.cand_u0.data_ptr(), s))

    def _result(self):
        G, K = self.G, self.K
        out = dict(u0=self.u0, cost=self.cost, winner=self.winner, cand_cost=self.cand_cost.view(G, K), cand_status=self.cand_status.view(G, K),
                   cand_iters=self.cand_iters.view(G, K), cand_u0=self.cand_u0.view(G, K, 2))
        if self.select_by == "rollout":
            out.update(cand_merit=self.cand_merit.view(G, K), cand_defect=self.cand_defect.view(G, K), cand_margin=self.cand_margin.view(G, K))
        return out

    def _on_stream(self):
        torch = self._torch
        outer = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(outer)
        return outer, torch.cuda.stream(self.stream)

    def solve(self, x0, obstacles, goal, keep_first=False, keep_solution=False):
        """One group solve: seed the K candidates of every scenario (keep_first: member 0 keeps the iterate it holds, the closed loop's warm start), ONE
        solve launch over all scenarios * K members, select with broadcast -- behind it every member of a group holds the winner's iterate.
        x0 (G, 5), obstacles (G, n_obst, 4) = (x, y, vx, vy), goal (G, 2).  Returns device tensors that the next call overwrites: per scenario u0 (G, 2),
        cost (G,), winner (G,) int32 (-1: no eligible member; then cost = +inf, u0 = 0 and nothing was copied); per candidate cand_cost, cand_status,
        cand_iters (G, K) and cand_u0 (G, K, 2).  select_by="rollout": the selection goes by the candidates' rollout merits, `cost` is the winner's merit, and
        the dict also holds cand_merit, cand_defect and cand_margin (G, K) (mpc_rollout_merit_dev).  keep_solution: solved_X / solved_U keep a copy of every member's iterate in front of the broadcast."""
        outer, ctx = self._on_stream()
        with ctx:
            self._solve(x0, obstacles, goal, True, keep_first, keep_solution, self.stream.cuda_stream)
        outer.wait_stream(self.stream)
        return self._result()

    def step(self, x, obst, goal, noise=None, randomness=0.1, vmax=2.0, keep_solution=False):
        """One closed-loop control step of every scenario, composed from the existing entry points: the group solve (the first step seeds every member,
        later ones solve what the last step left: member 0 the shifted winner, members 1 .. K - 1 reseeded) -> plant step of the G states with the
        winners' u0, x updated in place -> obstacle step, obst updated in place (noise (G, n_obst, 2) standard normals or None) -> shift of all members
        (behind the broadcast they all hold the winner) -> reseed of members 1 .. K - 1 around the new state; a group without a winner applies u = 0
        and is reseeded whole.  x (G, 5), obst (G, n_obst, 4) float64 device tensors, goal (G, 2).  Returns solve()'s dict."""
        torch = self._torch
        if not (isinstance(x, torch.Tensor) and isinstance(obst, torch.Tensor) and x.is_contiguous() and obst.is_contiguous()
                and x.dtype == torch.float64 and obst.dtype == torch.float64):
            raise ValueError("step updates x and obst in place: contiguous float64 device tensors")
        outer, ctx = self._on_stream()
        m, G, K = self.inner, self.G, self.K
        with ctx:
            s = self.stream.cuda_stream
            self._solve(x, obst, goal, not self._warm, False, keep_solution, s)
            m.plant_step_dev(G, x, self.u0, self._xn, stream=s)
            x.copy_(self._xn)
            m.obstacle_step_dev(G * self.n_obst, obst, None if noise is None else self._dev(noise).contiguous(), randomness, vmax, stream=s)
            m.shift_dev(self.B, self.X, self.U, stream=s)
            goal_rows = self._goal[:, 0].contiguous()
            self._seed(x, goal_rows, True, s, obst)
            # a group without a winner: member 0 too starts again, from its own guess of the family (offsets[0]), selected on the device
            _lib.check(_lib.lib().mpc_seed_guesses_dev(m._h, G, 1, x.data_ptr(), goal_rows.data_ptr(), self.offsets.data_ptr(), 0,
                                                       self._X1.data_ptr(), self._U1.data_ptr(), s))
            lost = (self.winner < 0)[:, None, None]
            X0, U0 = self.X.view(G, K, self.N + 1, 5)[:, 0], self.U.view(G, K, self.N, 2)[:, 0]
            X0.copy_(torch.where(lost, self._X1, X0)); U0.copy_(torch.where(lost, self._U1, U0))
            self._warm = True
        outer.wait_stream(self.stream)
        return self._result()

    # ------------------------------------------------------------------ the fused control step (mpc_group_step_dev)
    def _group_arrays(self):
        """the group bookkeeping of the fused step, the members' flag words and the scratch words of the member solve, made on first use"""
        if getattr(self, "ep_flags", None) is None:
            torch, G, B = self._torch, self.G, self.B
            f64 = dict(dtype=torch.float64, device=self.dev); i32 = dict(dtype=torch.int32, device=self.dev)
            self.min_margin, self.ep_flags, self.ep_steps = torch.full((G,), float("inf"), **f64), torch.zeros(G, **i32), torch.zeros(G, **i32)
            self.lost_steps, self.switched_steps = torch.zeros(G, **i32), torch.zeros(G, **i32)
            self.member_flags, self._scratch_margin, self._scratch_steps = torch.zeros(B, **i32), torch.full((B,), float("inf"), **f64), torch.zeros(B, **i32)
            p = lambda t: t.data_ptr()
            self._out = _lib.GroupStepOut(winner=p(self.winner), best_key=p(self.cost), best_u0=p(self.u0), min_margin=p(self.min_margin), ep_flags=p(self.ep_flags),
                                          ep_steps=p(self.ep_steps), lost=p(self.lost_steps), switched=p(self.switched_steps), member_x=p(self._x0),
                                          member_obst=p(self._obst), member_goal=p(self._goal), member_flags=p(self.member_flags))

    def restart(self):
        """forget the closed loop: the next step / step_fused seeds every member again, and the fused step's bookkeeping starts over (margin +inf, flags, steps
        and counters 0)"""
        self._warm = self._fused_warm = False
        if getattr(self, "ep_flags", None) is not None:
            with self._torch.cuda.stream(self.stream):
                self.min_margin.fill_(float("inf")); self._scratch_margin.fill_(float("inf"))
                for t in (self.ep_flags, self.ep_steps, self.lost_steps, self.switched_steps, self.member_flags, self._scratch_steps):
                    t.zero_()
            self.stream.synchronize()

    def members_loaded(self):
        """say that the members ARE loaded: something else (mpc_group_refill_dev, run_multistart_sweep) has written every member's iterate, the replicated
        member inputs and member_flags on the device, so the next step_fused solves what it finds instead of loading and seeding the members from its
        arguments.  restart() takes it back."""
        self._group_arrays()
        self._warm = self._fused_warm = True

    def step_fused(self, x, obst, goal, noise=None, randomness=0.1, vmax=2.0, margin_all=False):
        """step() with everything behind the solve in ONE launch (mpc_group_step_dev) and the episode bookkeeping per group on the device: a control step is
        the member solve (closed_loop_step_dev with flags = STEP_METRICS alone on the members' own flag words: members of a finished group idle) ->
        [select_by="rollout": predict_dev on the G scenario rows, rollout_merit_dev on the members] -> the group tail: select, plant (x in place), obstacles
        (obst in place, noise (G, n_obst, 2) standard normals as a contiguous float64 device tensor, or None), bookkeeping, next iterates, the members'
        inputs.  The FIRST call (and the first after restart()) loads the members from x, obst, goal and seeds every member; every later call solves what
        the last one left, so x, obst and goal must then be the tensors that call was given (step() and step_fused() are not to be mixed without a restart()
        between them: step() does not maintain the members' inputs; members_loaded() in front of the first call skips its load).  A group whose ep_flags bit 0 is set is neither solved nor
        stepped.  Returns step()'s dict and the group bookkeeping: min_margin, ep_flags, ep_steps, lost_steps, switched_steps (G,)."""
        torch = self._torch
        for t in (x, obst, goal) + (() if noise is None else (noise,)):
            if not (isinstance(t, torch.Tensor) and t.is_contiguous() and t.dtype == torch.float64 and t.is_cuda):
                raise ValueError("step_fused works in place and without copies: x, obst, goal and noise are contiguous float64 device tensors")
        check_group_shapes(self.G, self.n_obst, x, obst, goal)
        if noise is not None and tuple(noise.shape) != (self.G, self.n_obst, 2):
            raise ValueError(f"noise must be {(self.G, self.n_obst, 2)}, got {tuple(noise.shape)}")
        self._group_arrays()
        outer, ctx = self._on_stream()
        m, G, K, B = self.inner, self.G, self.K, self.B
        with ctx:
            s = self.stream.cuda_stream
            if not (self._warm and self._fused_warm):
                self._load(x, obst, goal)
                self.member_flags.copy_((self.ep_flags & 1).repeat_interleave(K))
                self._seed(x, goal, False, s, obst)
                self._warm = self._fused_warm = True
            m.closed_loop_step_dev(B, self._x0, self._obst, self._goal, self.X, self.U, self.cand_u0, self.cand_cost, self.cand_status, self.cand_iters,
                                   flags=_lib.STEP_METRICS, min_margin=self._scratch_margin, ep_flags=self.member_flags, ep_steps=self._scratch_steps, stream=s)
            by = self._select_key(x, obst, goal, s)
            rec = (G, K, x, obst, self.X, by, self.cand_status, self.cand_iters, self.cand_u0, self._out) if self._recording else None
            if rec is not None:          # what the group chooses among: the tail below overwrites it
                m.group_record_dev(rec[0], rec[1], _lib.GROUP_RECORD_SOLVED, *rec[2:], stream=s)
            _lib.check(_lib.lib().mpc_group_step_dev(m._h, G, K, by.data_ptr(), self.cand_status.data_ptr(), self.cand_u0.data_ptr(), self.margin,
                                                     _lib.GROUP_MARGIN_ALL if margin_all else 0, x.data_ptr(), obst.data_ptr(), goal.data_ptr(),
                                                     self.offsets.data_ptr(), None if noise is None else noise.data_ptr(), randomness, vmax,
                                                     self.X.data_ptr(), self.U.data_ptr(), self._out, s))
            if rec is not None:          # what it chose, and the states that left it in
                m.group_record_dev(rec[0], rec[1], _lib.GROUP_RECORD_STEPPED, *rec[2:], stream=s)
        outer.wait_stream(self.stream)
        return dict(self._result(), min_margin=self.min_margin, ep_flags=self.ep_flags, ep_steps=self.ep_steps, lost_steps=self.lost_steps,
                    switched_steps=self.switched_steps)

    def group_record_set_dev(self, rows=0, max_steps=0, **arrays):
        """attach a per-group record to the fused control step (BatchedMpc.group_record_set_dev with this object's K; the arrays by their names in
        BatchedMpc.GROUP_RECORD_FIELDS, device tensors used in place): while one is attached, step_fused launches mpc_group_record_dev twice per control step --
        SOLVED between the member solve (and the rollout merit) and the group tail, STEPPED behind the tail -- and with none attached exactly what it launches
        without this feature.  rows 0 (the default) detaches: group_record_off().  The non-fused step() records nothing."""
        if int(rows) == 0:
            return self.group_record_off()
        self.inner.group_record_set_dev(rows, max_steps, self.K, **arrays)
        self._recording = True

    def group_record_off(self):
        """detach the per-group record (the handle keeps no pointer into its arrays)"""
        self._recording = False
        self.inner.group_record_set_dev(0)

    def iterates(self):
        """the iterates of all members as they stand, (G, K, N + 1, 5) and (G, K, N, 2) device views"""
        return self.X.view(self.G, self.K, self.N + 1, 5), self.U.view(self.G, self.K, self.N, 2)


# ---------------------------------------------------------------------------------------------------------------------- the group drivers' argument checks
def _check_n_obst(n_obst):
    if isinstance(n_obst, bool) or int(n_obst) != n_obst or not 1 <= int(n_obst) <= 32:
        raise ValueError(f"n_obst must be a whole number in 1 .. 32, got {n_obst!r}")
    return int(n_obst)


def _check_sqp(sqp):
    if sqp is not None and (not hasattr(sqp, "__len__") or len(sqp) != 2):
        raise ValueError("sqp must be None or (max_iter, step_tol)")


def _check_solver(solver, G, off, margin, select_by, geometry, n_obst=None):
    """a caller's handle (None: the driver makes its own) is the one the call asks for: G groups, the offsets, margin, select_by and guess geometry; n_obst
    given: that obstacle count too (a batch of groups has its own; a sweep takes the handle's) -- or ValueError, in the words of the driver that asks"""
    if solver is None:
        return
    if not isinstance(solver, MultiStartMpc):
        raise ValueError("solver must be a MultiStartMpc (the groups' own handle)")
    holds = f"offsets {solver.offsets_host.tolist()}, margin {solver.margin}, select_by {solver.select_by!r}"
    if (solver.G != G or (n_obst is not None and solver.n_obst != n_obst) or solver.offsets_host.tolist() != off.tolist() or solver.margin != margin
            or solver.select_by != select_by):
        if n_obst is not None:
            raise ValueError(f"solver holds {solver.G} groups of {solver.n_obst} obstacles, {holds}: not what this call asks for")
        raise ValueError(f"solver holds {solver.G} groups, {holds}: this call asks for {G} group slots, offsets {off.tolist()}, margin {margin}, select_by {select_by!r}")
    if solver.guess_geometry != geometry:
        raise ValueError(f"solver has guess_geometry {solver.guess_geometry}: this call asks for {geometry}")


# ---------------------------------------------------------------------------------------------------------------------- episodes of groups
def episode_arguments(x0, goal, obst, offsets=DEFAULT_OFFSETS, incumbent_margin=0.0, select_by="cost", n_obst=5, max_iter=400, random_move=True, first_seed=0,
                      noise=None, sqp=None, r_safe=None, r_hit=None, active=None, solver=None, guess_geometry=None):
    """run_multistart_episodes' arguments, checked on the host before anything touches a device.  Returns dict(G, K, n_obst, x0 (G, 5), goal (G, 2), obst (the
    array (G, n_obst, 4) or None), scenario (the name or None), offsets, margin, select_by, max_iter, noise (None, "reference", "torch" or the array), first_seed,
    guess_geometry (None or check_guess_geometry's dict))."""
    from .episodes import _episode_noise
    off, margin, select_by = check_offsets(offsets), check_margin(incumbent_margin), check_select_by(select_by)
    geometry = check_guess_geometry(guess_geometry)
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    if x0.ndim != 2 or x0.shape[1] != 5 or x0.shape[0] < 1:
        raise ValueError(f"x0 must be (G, 5) with one row per group (G >= 1), got {x0.shape}")
    G, K = x0.shape[0], int(off.shape[0])
    try:
        goal = np.ascontiguousarray(np.broadcast_to(np.asarray(goal, dtype=np.float64), (G, 2)))
    except ValueError:
        raise ValueError(f"goal must be (2,) or ({G}, 2), got {np.shape(goal)}") from None
    scenario = obst if isinstance(obst, str) else None
    if scenario is not None:
        if scenario not in BatchedMpc.SCENARIOS:
            raise ValueError(f"unknown scenario {scenario!r}: one of {sorted(BatchedMpc.SCENARIOS)}")
        n_obst, obst = _check_n_obst(n_obst), None
    else:
        obst = np.ascontiguousarray(obst, dtype=np.float64)
        if obst.ndim != 3 or obst.shape[0] != G or obst.shape[2] != 4 or not 1 <= obst.shape[1] <= 32:
            raise ValueError(f"obst must be a scenario name or ({G}, n_obst, 4) with 1 .. 32 obstacles, got {obst.shape}")
        n_obst = obst.shape[1]
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or int(max_iter) < 1:
        raise ValueError(f"max_iter must be a whole number >= 1, got {max_iter!r}")
    if isinstance(first_seed, bool) or int(first_seed) != first_seed or not 0 <= int(first_seed) or int(first_seed) + G > 2 ** 32:
        raise ValueError("first_seed .. first_seed + G - 1 must be numpy seeds in [0, 2^32)")
    noise = _episode_noise(noise, scenario, 0, bool(random_move), int(max_iter), G, n_obst)
    _check_sqp(sqp)
    for name, a in (("r_safe", r_safe), ("r_hit", r_hit)):
        if a is not None:
            a = np.asarray(a, dtype=np.float64)
            if a.shape not in ((G,), (G, n_obst)) or not np.isfinite(a).all() or not (a > 0.0).all():
                raise ValueError(f"{name} must be ({G},) or ({G}, {n_obst}) finite radii > 0 (one row per group), got shape {a.shape}")
    if active is not None and (np.asarray(active).shape != (G, n_obst) or np.asarray(active).dtype != np.bool_):
        raise ValueError(f"active must be a bool array ({G}, {n_obst}) (one row per group), got {np.asarray(active).dtype} {np.asarray(active).shape}")
    _check_solver(solver, G, off, margin, select_by, geometry, n_obst=n_obst)
    return dict(G=G, K=K, n_obst=n_obst, x0=x0, goal=goal, obst=obst, scenario=scenario, offsets=off, margin=margin, select_by=select_by, max_iter=int(max_iter),
                noise=noise, first_seed=int(first_seed), guess_geometry=geometry)


def group_record_bytes(rows, max_iter, N, n_obst, K, plans=True):
    """device bytes of a per-group record (mpc_group_record): per recorded group x (max_iter + 1, 5), obst (max_iter + 1, n_obst, 4), u (max_iter, 2), best_key
    (max_iter,), cand_key (max_iter, K), cand_u0 (max_iter, K, 2) and, with plans, cand_X (max_iter, K, N + 1, 5) in float64; winner (max_iter,), cand_status and
    cand_iters (max_iter, K) and one len word in int32"""
    rows, T, N, n_obst, K = int(rows), int(max_iter), int(N), int(n_obst), int(K)
    per_row = 8 * ((T + 1) * 5 + (T + 1) * n_obst * 4 + T * 2 + T + T * K + T * K * 2 + (T * K * (N + 1) * 5 if plans else 0)) + 4 * (T + 2 * T * K + 1)
    return rows * per_row


def _group_record(G, max_iter, N, n_obst, K, record=None, record_plans=True, record_max_bytes=2 ** 31):
    """run_multistart_episodes' record arguments, checked on the host before anything touches a device, by the rules of episodes._sweep_trace.  Returns None
    (no record) or dict(groups: the recorded group indices (rows,) in the order given, group_row: int32 (G,) = the row of each group or -1, plans, bytes)."""
    if record is None or record is False:
        return None
    if not isinstance(record_plans, (bool, np.bool_)):
        raise ValueError("record_plans must be True or False")
    if isinstance(record_max_bytes, (bool, np.bool_)) or not isinstance(record_max_bytes, (int, np.integer)) or record_max_bytes < 0:
        raise ValueError("record_max_bytes must be a whole number of bytes >= 0")
    what = f"record must be None, True or a sequence of group indices in 0 .. {G - 1}"
    if record is True:
        groups = np.arange(G, dtype=np.int64)
    else:
        if isinstance(record, (str, bytes, dict, set, frozenset)) or not hasattr(record, "__len__"):
            raise ValueError(what)
        try:
            a = np.asarray(record)
        except Exception:
            raise ValueError(what) from None
        if a.ndim != 1 or a.size == 0 or a.dtype.kind not in "iu":
            raise ValueError(f"record must be a non-empty 1-d sequence of whole group indices (0 .. {G - 1}), got {a.dtype} {a.shape}")
        if (a < 0).any() or (a >= G).any():
            raise ValueError(f"record holds a group index outside 0 .. {G - 1}: {a[(a < 0) | (a >= G)][0]}")
        groups = a.astype(np.int64)
        if np.unique(groups).size != groups.size:
            raise ValueError("record names a group index twice (every recorded group owns one row)")
    need = group_record_bytes(groups.size, max_iter, N, n_obst, K, plans=bool(record_plans))
    if need > record_max_bytes:
        raise ValueError(f"record: the arrays of {groups.size} groups x {int(max_iter)} control steps x {int(K)} members take {need} bytes, more than "
                         f"record_max_bytes = {int(record_max_bytes)}: record fewer groups"
                         + (" or pass record_plans=False (the candidates' plans are most of it)" if record_plans else ""))
    group_row = np.full(G, -1, dtype=np.int32)
    group_row[groups] = np.arange(groups.size, dtype=np.int32)
    return dict(groups=groups, group_row=group_row, plans=bool(record_plans), bytes=need)


def _group_lease(solver, make):
    """episodes._HandleLease for a MultiStartMpc: the setters it undoes, and the per-group record's (group_record_set_dev(0) detaches)"""
    from .episodes import _HandleLease

    class _GroupLease(_HandleLease):
        OFF = dict(_HandleLease.OFF, group_record_set_dev=(0,))
    return _GroupLease(solver, make)


def _attach_group_record(lease, torch, rc, max_iter):
    """the per-group rows (mpc_group_record) on the lease's MultiStartMpc: row r belongs to group rc["groups"][r].  Returns the arrays by their names in
    group_record_set_dev"""
    ms = lease.m
    R, N, no, K, T = rc["groups"].size, ms.N, ms.n_obst, ms.K, int(max_iter)
    f64 = dict(dtype=torch.float64, device=ms.dev); i32 = dict(dtype=torch.int32, device=ms.dev)
    arr = dict(group_row=torch.from_numpy(rc["group_row"]).to(ms.dev), len=torch.zeros(R, **i32), x=torch.zeros(R, T + 1, 5, **f64),
               obst=torch.zeros(R, T + 1, no, 4, **f64), u=torch.zeros(R, T, 2, **f64), winner=torch.zeros(R, T, **i32), best_key=torch.zeros(R, T, **f64),
               cand_key=torch.zeros(R, T, K, **f64), cand_status=torch.zeros(R, T, K, **i32), cand_iters=torch.zeros(R, T, K, **i32),
               cand_u0=torch.zeros(R, T, K, 2, **f64), cand_X=torch.zeros(R, T, K, N + 1, 5, **f64) if rc["plans"] else None)
    lease.attach("group_record_set_dev", R, T, **arr)
    return arr


_RECORD_CUT = dict(simX=("x", 1), obst_traj=("obst", 1), u=("u", 0), winner=("winner", 0), key=("best_key", 0), cand_key=("cand_key", 0),
                   cand_status=("cand_status", 0), cand_iters=("cand_iters", 0), cand_u0=("cand_u0", 0), cand_X=("cand_X", 0))      # name -> (array, rows beyond L)


def _collect_group_record(arr, rc, table):
    """the recorded rows on the host, once the stream has drained, cut to each group's length and held to the table's lengths"""
    th = {n: t.cpu().numpy() for n, t in arr.items() if t is not None and n != "group_row"}
    want = (table[rc["groups"], 4] + table[rc["groups"], 1]).astype(np.int64)
    if not np.array_equal(th["len"], want):
        bad = np.nonzero(th["len"] != want)[0]
        raise _lib.MpcError(f"record: group {int(rc['groups'][bad[0]])} recorded {int(th['len'][bad[0]])} control steps, its table row says {int(want[bad[0]])}")
    return {g: {n: th[src][r, :int(th["len"][r]) + more].copy() for n, (src, more) in _RECORD_CUT.items() if src in th} for r, g in enumerate(rc["groups"].tolist())}


def multistart_record(result, g, member=None):
    """One recorded group of run_multistart_episodes(..., record=...) in run_episodes(record=True)'s layout, as a batch of one: dict(simX (L + 1, 1, 5),
    obst_traj (L + 1, 1, n_obst, 4), pred (L, 1, N + 1, 5), table (1, 6), x_last (1, 5)), so that visualisation_inputs(multistart_record(result, g), 0) is
    what the reference hands to its VisDynamicRobotEnv for that group.  pred[t] is the SOLVED plan of step t's winner -- of member 0 on a step without a
    winner --, or with member=k always candidate k's (the pass-left or pass-right plan next to the one chosen), written in the SHIFTED layout
    visualisation_inputs re-assembles (stage j at j - 1, stage N kept).  Needs record_plans=True."""
    rec = result.get("record") if isinstance(result, dict) else None
    if rec is None:
        raise ValueError("the episodes were run without a record: pass record=True or the group indices to run_multistart_episodes")
    if isinstance(g, (bool, np.bool_)) or not isinstance(g, (int, np.integer)) or int(g) not in rec:
        raise ValueError(f"group {g!r} was not recorded (recorded: {sorted(rec)[:8]}{' ...' if len(rec) > 8 else ''})")
    t = rec[int(g)]
    if "cand_X" not in t:
        raise ValueError("the record holds no plans (record_plans=False): a record for visualisation_inputs needs them")
    L, K, N1 = t["cand_X"].shape[:3]
    if member is None:
        pick = np.where(t["winner"] >= 0, t["winner"], 0).astype(np.int64)
    else:
        if isinstance(member, (bool, np.bool_)) or not isinstance(member, (int, np.integer)) or not 0 <= int(member) < K:
            raise ValueError(f"member must be None (the winner's plan) or a candidate in 0 .. {K - 1}, got {member!r}")
        pick = np.full(L, int(member), dtype=np.int64)
    solved = t["cand_X"][np.arange(L), pick]                                            # (L, N + 1, 5)
    pred = solved[:, np.minimum(np.arange(N1) + 1, N1 - 1)]                             # stage j at j - 1, stage N kept
    return dict(simX=t["simX"][:, None].copy(), obst_traj=t["obst_traj"][:, None].copy(), pred=pred[:, None].copy(),
                table=np.array(result["table"][int(g)][None]), x_last=np.array(result["x_last"][int(g)][None]))


def run_multistart_episodes(x0, goal, obst, offsets=DEFAULT_OFFSETS, incumbent_margin=0.0, select_by="cost", N=20, Tf=2.0, n_obst=5, max_iter=400, random_move=True,
                            first_seed=0, noise=None, sqp=None, r_safe=None, r_hit=None, active=None, margin_all=False, solver=None, device=0,
                            guess_geometry=None, record=None, record_plans=True, record_max_bytes=2 ** 31, **cfg):
    """run_episodes for GROUPS: G closed-loop episodes of K = len(offsets) candidate iterates each, one MultiStartMpc.step_fused per control step (noise draw ->
    member solve -> [predict, rollout merit] -> group tail), episode bookkeeping per group on the device.  x0 (G, 5), goal (2,) or (G, 2), obst (G, n_obst, 4)
    -- or a scenario name ("RANDOM" | "CENTER" | "EDGE"): group s is then the reference's episode for np.random.seed(first_seed + s) (experiments.py:20-36), its
    scenario draw and its noise stream produced on the device (mpc_generate_scenarios_dev, mpc_noise_init_dev, mpc_noise_draw_dev over the G scenario rows with
    the GROUP flags: a finished group draws no more).  The plant starts from x0 as given.
    noise: as run_episodes -- an array (>= max_iter, G, n_obst, 2), "reference" (the default with a scenario name), "torch" (the default with explicit
    obstacle states); random_move=False: the obstacles draw nothing.  sqp (max_iter, step_tol), r_safe / r_hit ((G,) or (G, n_obst)), active (bool (G, n_obst))
    with margin_all: per GROUP, as run_episodes takes them per instance (MultiStartMpc replicates them over the members).  guess_geometry: as MultiStartMpc
    takes it (the amplitudes of the seeded members from the obstacles in the way, formed by the group tail on the new state and the moved obstacles).
    A group that has reached its goal is neither solved nor stepped.  The loop ends as run_episodes' does: every 25 control steps the
    done flag goes to pinned host memory behind an event and is looked at once that event has passed -- no stall, at most ~25 steps on idle groups.
    solver: a caller's MultiStartMpc with the same groups, offsets, margin and select_by; it is restart()ed, and leaves with the features of this call switched
    OFF again whether the call returns or raises (_HandleLease).  The arguments that need no device are checked before a handle is touched (episode_arguments).
    record: None (off, the default), True (every group) or a sequence of group INDICES in 0 .. G-1 without duplicates: the closed-loop record of those groups,
    written on the device (mpc_group_record_set_dev / mpc_group_record_dev: two small launches per control step, in front of and behind the group tail, which
    selects the winner and overwrites the candidates in one launch).  `record` in the result is a dict keyed by group index; with L = the
    group's control steps (= table[g, 4] + table[g, 1]) each value holds simX (L + 1, 5), obst_traj (L + 1, n_obst, 4), u (L, 2) = the input applied, winner (L,)
    (-1: no member was eligible, u = 0), key (L,) = the winner's key, and per candidate cand_key (the reported cost, or the rollout merit), cand_status,
    cand_iters (L, K), cand_u0 (L, K, 2) and, unless record_plans=False, cand_X (L, K, N + 1, 5): every member's SOLVED plan, stage j at row j.
    multistart_record(result, g) puts one group into run_episodes(record=True)'s layout for visualisation_inputs.  The arrays take
    group_record_bytes(rows, max_iter, N, n_obst, K, record_plans) device bytes (1.1 MB per group with plans and 0.13 MB without, at max_iter 400, N 20,
    5 obstacles and K 3); above record_max_bytes the call is refused on the host.  table, x_last, lost_steps and switched_steps are those of the call without a
    record, bit for bit.
    Not offered: PipelinedMpc, compaction, a record of the non-fused step().  More seeds than groups, or groups that do not idle once their
    episode has ended: run_multistart_sweep (the refill for groups; it takes no record: the record is keyed by group).
    Returns dict(table (G, 6) = [hit, reached, min_margin, dist_to_goal, iters, out_of_bounds] (episodes.result_table), x_last (G, 5), steps_run, solves = the
    member solves of running groups = K (sum of table[:, 4] + table[:, 1]), lost_steps (G,): control steps on which no member was eligible, switched_steps (G,):
    control steps on which the winner was not member 0), and with record: record)."""
    from .episodes import _episode_loop, _noise_source, result_table
    from types import SimpleNamespace
    a = episode_arguments(x0, goal, obst, offsets, incumbent_margin, select_by, n_obst, max_iter, random_move, first_seed, noise, sqp, r_safe, r_hit, active, solver,
                          guess_geometry)
    rc = _group_record(a["G"], a["max_iter"], solver.N if solver is not None else int(N), a["n_obst"], a["K"], record, record_plans, record_max_bytes)
    import torch
    G, K, no = a["G"], a["K"], a["n_obst"]
    dev = torch.device("cuda", device if solver is None else solver.dev.index)
    make = lambda: MultiStartMpc(N, no, Tf, scenarios=G, offsets=a["offsets"], incumbent_margin=a["margin"], device=device, select_by=a["select_by"],
                                 guess_geometry=a["guess_geometry"], **cfg)
    with _group_lease(solver, make) as lease:
        ms = lease.m
        lease.stream = ms.stream
        if r_safe is not None or r_hit is not None:
            lease.attach("set_instance_params", r_safe=r_safe, r_hit=r_hit)
        if active is not None:
            lease.attach("set_obstacle_mask", np.asarray(active))
        if sqp is not None:
            lease.attach("set_sqp", *sqp)
        ms.restart()
        with torch.cuda.stream(ms.stream):
            s = ms.stream.cuda_stream
            f64 = dict(dtype=torch.float64, device=dev)
            x, dgoal = torch.from_numpy(a["x0"].copy()).to(dev), torch.from_numpy(a["goal"].copy()).to(dev)
            if a["scenario"] is not None:
                dobst = torch.zeros(G, no, 4, **f64)
                ms.inner.generate_scenarios_dev(a["scenario"], G, dobst, seed0=a["first_seed"], stream=s)
            else:
                dobst = torch.from_numpy(a["obst"].copy()).to(dev)
            ms._group_arrays()
            rarr = _attach_group_record(lease, torch, rc, a["max_iter"]) if rc is not None else None
            rows = SimpleNamespace(rows=G, obst=dobst, flags=ms.ep_flags, f64=f64, gen_state=None, nbuf=None)
            draw = _noise_source(torch, ms.inner, rows, a["noise"], a["scenario"], a["first_seed"], 0, s)
            def step(k):
                nz = draw(k)
                ms.step_fused(x, dobst, dgoal, noise=None if nz is None else nz.contiguous(), margin_all=bool(margin_all) and active is not None)
            k = _episode_loop(torch, ms.stream, a["max_iter"], step, lambda: ms.ep_flags)
            ms.stream.synchronize()
            xl = x.cpu().numpy()
            table = result_table(ms.ep_flags.cpu().numpy(), ms.min_margin.cpu().numpy(), xl, a["goal"], ms.ep_steps.cpu().numpy())
            lost, switched = ms.lost_steps.cpu().numpy().copy(), ms.switched_steps.cpu().numpy().copy()
            rec = {} if rarr is None else dict(record=_collect_group_record(rarr, rc, table))
    return dict(table=table, x_last=xl, steps_run=k, solves=K * int(table[:, 4].sum() + table[:, 1].sum()), lost_steps=lost, switched_steps=switched, **rec)


# ---------------------------------------------------------------------------------------------------------------------- seed sweeps of groups
_SWEEP_NOT_OFFERED = ("r_safe", "r_hit", "W", "We", "active", "margin_all", "bounds", "status_log", "ring", "ring_every", "trace", "trace_pred", "trace_max_bytes",
                      "record", "noise", "seed", "first_seed", "compact_from")


def sweep_arguments(start, goal, scenario, seeds, slots, offsets=DEFAULT_OFFSETS, incumbent_margin=0.0, select_by="cost", n_obst=5, max_iter=400, sqp=None,
                    poll_every=25, solver=None, guess_geometry=None):
    """run_multistart_sweep's arguments, checked on the host before anything touches a device.  Returns dict(first, count, start (rows, 5), goal (rows, 2),
    per_seed, S = the group slots used, K, n_obst, offsets, margin, select_by, max_iter, poll_every, bound = the control steps the loop launches at most,
    guess_geometry = None or check_guess_geometry's dict)."""
    from .episodes import _sweep_arguments
    off, margin, select_by = check_offsets(offsets), check_margin(incumbent_margin), check_select_by(select_by)
    geometry = check_guess_geometry(guess_geometry)
    first, count, start, goal, per_seed = _sweep_arguments(start, goal, scenario, seeds, slots, max_iter, poll_every)
    n_obst = _check_n_obst(n_obst)
    _check_sqp(sqp)
    S, K = min(int(slots), count), int(off.shape[0])
    _check_solver(solver, S, off, margin, select_by, geometry)
    if solver is not None:
        n_obst = solver.n_obst
    return dict(first=first, count=count, start=start, goal=goal, per_seed=per_seed, S=S, K=K, n_obst=int(n_obst), offsets=off, margin=margin, select_by=select_by,
                max_iter=int(max_iter), poll_every=int(poll_every), bound=-(-count // S) * int(max_iter) + int(poll_every), guess_geometry=geometry)


def _sweep_state(torch, ms, a, scenario, random_move=True):
    """the device state of a sweep of groups on the MultiStartMpc `ms` (restart()ed), on the current stream: the start and goal rows, the group rows x, obst,
    goal, the generator states and the noise they draw into (nbuf; None: the obstacles draw nothing), slot_seed, cursor and the result rows of a["count"]
    seeds, all preset as the first call of a sweep wants them (every group "finished" and without a seed: the first refill fills them all; the members
    count as loaded); `refill(stream)` is one mpc_group_refill_dev call on them and the handle's own group and member arrays.  a: sweep_arguments' dict."""
    from types import SimpleNamespace
    S, no, count, dev = a["S"], ms.n_obst, a["count"], ms.dev
    f64 = dict(dtype=torch.float64, device=dev); i32 = dict(dtype=torch.int32, device=dev)
    st = SimpleNamespace(start_rows=torch.from_numpy(a["start"]).to(dev), goal_rows=torch.from_numpy(a["goal"]).to(dev), x=torch.zeros(S, 5, **f64),
                         obst=torch.zeros(S, no, 4, **f64), goal=torch.zeros(S, 2, **f64), state=torch.zeros(S, _lib.lib().mpc_noise_state_words(), **i32),
                         nbuf=torch.zeros(S, no, 2, **f64) if random_move else None, slot_seed=torch.full((S,), -1, **i32), cursor=torch.zeros(2, **i32),
                         res_f=torch.full((count, 6), float("nan"), **f64), res_i=torch.full((count, 4), -1, **i32), box=BatchedMpc._scenario_box())
    ms.members_loaded()
    ms.ep_flags.fill_(1); ms.member_flags.fill_(1)
    p = lambda t: t.data_ptr()
    st.arrays = _lib.GroupRefillArrays(x=p(st.x), obst=p(st.obst), goal=p(st.goal), X=p(ms.X), U=p(ms.U), min_margin=p(ms.min_margin), ep_flags=p(ms.ep_flags),
                                       ep_steps=p(ms.ep_steps), lost=p(ms.lost_steps), switched=p(ms.switched_steps), state=p(st.state), slot_seed=p(st.slot_seed),
                                       cursor=p(st.cursor), res_f=p(st.res_f), res_i=p(st.res_i), member_x=p(ms._x0), member_obst=p(ms._obst),
                                       member_goal=p(ms._goal), member_flags=p(ms.member_flags))
    st.refill = lambda stream: _lib.check(_lib.lib().mpc_group_refill_dev(ms.inner._h, S, ms.K, BatchedMpc.SCENARIOS[scenario], a["first"], count, a["max_iter"],
                                                                          st.box.ctypes.data, p(st.start_rows), p(st.goal_rows), 1 if a["per_seed"] else 0,
                                                                          p(ms.offsets), st.arrays, stream))
    return st


def run_multistart_sweep(start, goal, scenario, seeds, slots, offsets=DEFAULT_OFFSETS, incumbent_margin=0.0, select_by="cost", N=20, Tf=2.0, n_obst=5, max_iter=400,
                         random_move=True, sqp=None, poll_every=25, solver=None, device=0, guess_geometry=None, **cfg):
    """run_seed_sweep for GROUPS: the seeds stream through min(slots, count) GROUP slots of K = len(offsets) members each, and a group whose episode has ended
    (goal reached, or max_iter control steps spent) starts the next seed on the device, in front of the next member solve (mpc_group_refill_dev: no host
    read, no gather; a finished group does not idle in its K wavefront slots while seeds are left).  Seed index k is group k of
    run_multistart_episodes(start rows, goal, scenario, first_seed=first, ...) on ONE batch of `count` groups: the same scenario draw, noise stream, guesses
    and control steps -- the rows are those of that batch to the rounding of the wavefront sums (three member solves share a wavefront).
    scenario, seeds, start (5,) or (count, 5), goal (2,) or (count, 2), poll_every: as run_seed_sweep.  offsets, incumbent_margin, select_by, sqp, random_move:
    as run_multistart_episodes; guess_geometry too (the refill forms a started group's amplitudes from its start row and the obstacles it has just drawn).  One control step is refill -> poll copy -> noise draw on the group rows -> member solve -> [predict, rollout merit] -> group
    tail (MultiStartMpc.step_fused on members that are already loaded).  The loop ends as run_seed_sweep's does and launches at most
    ceil(count / S) * max_iter + poll_every control steps whatever the device returns.
    solver: a caller's MultiStartMpc with min(slots, count) groups and the same offsets, margin and select_by; it is restart()ed on entry and on exit, and
    leaves with the SQP setting of this call switched OFF again whether the call returns or raises (_HandleLease).
    Not offered (TypeError, as run_seed_sweep answers `record`): per-seed feature tables (r_safe, r_hit, W, We, active, bounds), status_log, ring, trace.
    Returns dict(table (count, 6), x_last (count, 5), steps_run, solves = K (sum of table[:, 4] + table[:, 1]), lost_steps (count,), switched_steps (count,),
    schedule): table as episodes.result_table builds it; schedule (count, 2) = group slot and control step at which each seed started (poll_every = 1; None
    otherwise) = refill_schedule's slot / start on the groups' episode lengths."""
    not_offered = sorted(set(cfg) & set(_SWEEP_NOT_OFFERED))
    if not_offered:
        raise TypeError(f"run_multistart_sweep has no argument {not_offered[0]!r}: per-seed feature tables, the status log, the ring and the trace are "
                        "run_seed_sweep's, and a batch's arguments are run_multistart_episodes'")
    a = sweep_arguments(start, goal, scenario, seeds, slots, offsets, incumbent_margin, select_by, n_obst, max_iter, sqp, poll_every, solver, guess_geometry)
    from .episodes import _HandleLease, _sweep_loop, _sweep_table
    import torch
    S, K, count, no, poll = a["S"], a["K"], a["count"], a["n_obst"], a["poll_every"]
    make = lambda: MultiStartMpc(N, no, Tf, scenarios=S, offsets=a["offsets"], incumbent_margin=a["margin"], device=device, select_by=a["select_by"],
                                 guess_geometry=a["guess_geometry"], **cfg)
    with _HandleLease(solver, make) as lease:
        ms = lease.m
        lease.stream = ms.stream
        if sqp is not None:
            lease.attach("set_sqp", *sqp)
        ms.restart()
        try:
            with torch.cuda.stream(ms.stream):
                s = ms.stream.cuda_stream
                st = _sweep_state(torch, ms, a, scenario, random_move)
                def step(k):
                    if st.nbuf is not None:
                        ms.inner.noise_draw_dev(S, st.state, st.nbuf, ep_flags=ms.ep_flags, stream=s)
                    ms.step_fused(st.x, st.obst, st.goal, noise=st.nbuf)
                k, schedule = _sweep_loop(torch, ms.stream, S, count, st.slot_seed, st.cursor, poll, a["bound"], lambda k: st.refill(s), step)
                ms.stream.synchronize()
                table, xl, ri = _sweep_table(st.cursor, st.res_i, st.res_f, a["goal"], a["bound"], "groups")
        finally:
            ms.restart()
    return dict(table=table, x_last=xl, steps_run=k, solves=K * int(table[:, 4].sum() + table[:, 1].sum()), lost_steps=ri[:, 2].copy(), switched_steps=ri[:, 3].copy(),
                schedule=schedule)
