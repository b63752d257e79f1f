"""MultiStartMpc: K initial guesses per scenario, the best kept on the device (include/mpc_gpu.h, MULTI-START).

The problem is non-convex: an obstacle on the line from robot to goal splits the solutions into "pass left" and "pass right", and an RTI / SQP iteration
stays in the family its guess sits in.  A MultiStartMpc of `scenarios` groups sits over ONE BatchedMpc of scenarios * K instances -- member k of group g is
instance g K + k, and every member of a group is given the group's x0, obstacles and goal -- and runs, per solve, three launches on one stream:

    mpc_seed_guesses_dev  ->  the ordinary solve launch (closed_loop_step_dev with flags = 0: the look-ahead fused)  ->  mpc_select_best_dev (broadcast)

select_by="rollout" puts two launches between the solve and the selection -- mpc_predict_dev on the G scenario rows and mpc_rollout_merit_dev on the members'
solved (X, U) with members = K -- and the selection then compares the candidates' ROLLOUT MERITS, the NLP objective of what the plant does under each U,
instead of the costs the solve reports for iterates that need not be dynamically consistent.

Nothing leaves the device between them: torch replicates the group inputs and carries the tensors, the `_dev` entry points do the work.  The pure helpers
(`check_offsets`, `check_margin`, `check_select_by`, `check_group_shapes`, `replicate`) import without a GPU.  run_episodes, run_seed_sweep and PipelinedMpc do not know
about groups."""
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

    def __init__(self, N=20, n_obst=3, Tf=2.0, scenarios=1, offsets=DEFAULT_OFFSETS, incumbent_margin=0.0, device=0, select_by="cost", **cfg):
        self.select_by = check_select_by(select_by)
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
        self.offsets = torch.from_numpy(off).to(self.dev)
        self.X, self.U = f64(B, N + 1, 5), f64(B, N, 2)                      # the iterates of all members
        self._x0, self._obst, self._goal = f64(G, K, 5), f64(G, K, no, 4), f64(G, K, 2)      # the group inputs, replicated per member
        self.cand_u0, self.cand_cost, self.cand_status, self.cand_iters = f64(B, 2), f64(B), i32(B), i32(B)
        self.winner, self.cost, self.u0 = i32(G), f64(G), f64(G, 2)
        self._xn, self._X1, self._U1 = f64(G, 5), f64(G, N + 1, 5), f64(G, N, 2)      # plant output; the reseed of member 0 of a failed group
        if self.select_by == "rollout":      # the scenarios' look-ahead (one row per group) and what the rollout reports per candidate
            self._P = f64(G, N + 1, no, 2)
            self.cand_merit, self.cand_defect, self.cand_margin = f64(B), f64(B), f64(B)
        self.solved_X = self.solved_U = None
        self._warm = False
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

    def _seed(self, x_rows, goal_rows, keep_first, s):
        """mpc_seed_guesses_dev from per-GROUP rows: x_rows (G, 5) and goal_rows (G, 2), contiguous"""
        _lib.check(_lib.lib().mpc_seed_guesses_dev(self.inner._h, self.G, self.K, x_rows.data_ptr(), goal_rows.data_ptr(), self.offsets.data_ptr(),
                                                   1 if keep_first else 0, self.X.data_ptr(), self.U.data_ptr(), s))

    def _solve(self, x0, obstacles, goal, seed, keep_first, keep_solution, s):
        self._load(x0, obstacles, goal)
        if seed:
            self._seed(self._x0[:, 0].contiguous(), self._goal[:, 0].contiguous(), keep_first, s)
        self.inner.closed_loop_step_dev(self.B, self._x0, self._obst, self._goal, self.X, self.U, self.cand_u0, self.cand_cost, self.cand_status,
                                        self.cand_iters, flags=0, stream=s)
        if keep_solution:
            self.solved_X, self.solved_U = self.X.clone(), self.U.clone()
        by = self.cand_cost
        if self.select_by == "rollout":
            self.inner.predict_dev(self.G, self._obst[:, 0].contiguous(), self._P, stream=s)
            self.inner.rollout_merit_dev(self.B, self._x0[:, 0].contiguous(), self._P, self._goal[:, 0].contiguous(), self.U, X=self.X, merit=self.cand_merit,
                                         defect=self.cand_defect, margin=self.cand_margin, members=self.K, stream=s)
            by = self.cand_merit
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
            self._seed(x, goal_rows, True, s)
            # a group without a winner: member 0 too starts again, from its own guess of the family (offsets[0]), selected on the device
            _lib.check(_lib.lib().mpc_seed_guesses_dev(m._h, G, 1, x.data_ptr(), goal_rows.data_ptr(), self.offsets.data_ptr(), 0,
                                                       self._X1.data_ptr(), self._U1.data_ptr(), s))
            lost = (self.winner < 0)[:, None, None]
            X0, U0 = self.X.view(G, K, self.N + 1, 5)[:, 0], self.U.view(G, K, self.N, 2)[:, 0]
            X0.copy_(torch.where(lost, self._X1, X0)); U0.copy_(torch.where(lost, self._U1, U0))
            self._warm = True
        outer.wait_stream(self.stream)
        return self._result()

    def iterates(self):
        """the iterates of all members as they stand, (G, K, N + 1, 5) and (G, K, N, 2) device views"""
        return self.X.view(self.G, self.K, self.N + 1, 5), self.U.view(self.G, self.K, self.N, 2)
