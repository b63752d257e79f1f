"""BatchedMpc: host-side owner of one libmpcgpu handle (one device, one stream, up to max_batch instances).

Mirrors what the reference keeps inside its `AcadosOcpSolver` object (iterate X, U; parameters; options) for the
solve path of src/simulation/robot_ocp_problem.py:186-198, batched over independent MPC instances.
"""
import ctypes as C
import os

import numpy as np

from . import _lib


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f"expected shape {tuple(shape)}, got {a.shape}")
    return a


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    if isinstance(a, np.ndarray):
        return C.c_void_p(a.ctypes.data)
    return C.c_void_p(a.data_ptr())      # torch tensor (device or host)


def _is_host(a):
    """a numpy array or a (nested) list / tuple, which a setter validates and copies; anything else is a device tensor, used in place"""
    return isinstance(a, (np.ndarray, list, tuple))


def _check_device(message, t, shape, dtypes=None, contiguous=True):
    """a device tensor that a setter uses in place (None: none given, nothing to check): its shape (None: any extent there), its dtype among `dtypes`
    (torch's names; None: not looked at) and, unless switched off, contiguity -- or ValueError(message)"""
    if t is None:
        return
    ok = len(t.shape) == len(shape) and all(want is None or have == want for have, want in zip(t.shape, shape))
    if not ok or (dtypes is not None and str(t.dtype) not in dtypes) or (contiguous and not t.is_contiguous()):
        raise ValueError(message)


def pack_obstacle_mask(active):
    """bool (B, n_obst) -> np.uint32 (B,): bit j of word b set iff active[b, j] (the words of mpc_set_obstacle_mask; n_obst <= 32)"""
    a = np.asarray(active)
    if a.ndim != 2 or a.shape[1] < 1 or a.shape[1] > 32:
        raise ValueError(f"active must be a bool array (B, n_obst) with 1 <= n_obst <= 32, got shape {a.shape}")
    if a.dtype != np.bool_:
        if not np.isin(a, (0, 1)).all():
            raise ValueError("active must hold booleans (or 0 / 1)")
        a = a.astype(np.bool_)
    w = (a.astype(np.uint64) << np.arange(a.shape[1], dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    return np.ascontiguousarray(w.astype(np.uint32))


def mask_rows(active, n_obst, rows="B", why=""):
    """a per-instance obstacle mask as an array (rows, n_obst), shape checked; `rows` is the caller's word for the row count and `why` ends its message"""
    a = np.asarray(active)
    if a.ndim != 2 or a.shape[1] != n_obst:
        raise ValueError(f"active must be ({rows}, {n_obst}), got {a.shape}" + why)
    return a


# the per-instance arrays of mpc_set_instance_params in the order of the C prototype: (name, columns -- None: n_obst, and (rows,) means one radius per instance)
INSTANCE_ROW = (("W", 6), ("We", 4), ("r_safe", None), ("r_hit", None))


def instance_rows(name, a, cols, n_obst, rows="B"):
    """one per-instance array of set_instance_params as contiguous float64 (rows, cols); a radius array (cols None) has n_obst columns and may be (rows,),
    one radius per instance.  `rows` is the caller's word for the row count; values are not looked at."""
    radius, cols = cols is None, n_obst if cols is None else cols
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1 and radius:
        a = np.repeat(a[:, None], n_obst, axis=1)
    if a.ndim != 2 or a.shape[1] != cols:
        raise ValueError(f"{name} must be ({rows}, {cols})" + (f" or ({rows},)" if radius else "") + f", got {a.shape}")
    return np.ascontiguousarray(a)


def unpack_obstacle_mask(words, n_obst):
    """np.uint32 (B,) -> bool (B, n_obst): the inverse of pack_obstacle_mask"""
    w = np.asarray(words, dtype=np.uint32).astype(np.uint64)
    return ((w[:, None] >> np.arange(int(n_obst), dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.bool_)


# one row of the packed bounds table of mpc_set_instance_bounds_dev: (name, first column, columns)
BOUNDS_ROW = (("bu_lo", 0, 2), ("bu_hi", 2, 2), ("bx_lo", 4, 4), ("bx_hi", 8, 4))
BOUNDS_COLS = 12


def _bounds_group(name, a, cols, B=None, rows="B"):
    """one group of instance bounds as a float64 (B, cols) array; a single row (cols,) is broadcast to B rows (B None: stays one row).  `rows` is the
    caller's word for the row count."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1 and a.shape == (cols,):
        a = np.tile(a[None, :], (1 if B is None else B, 1))
    if a.ndim != 2 or a.shape[1] != cols:
        raise ValueError(f"{name} must be ({rows}, {cols}) or ({cols},), got {a.shape}")
    if B is not None and a.shape[0] != B:
        raise ValueError(f"{name} has {a.shape[0]} rows, expected {B}")
    return np.ascontiguousarray(a)


def pack_instance_bounds(cfg, B, bx_lo=None, bx_hi=None, bu_lo=None, bu_hi=None, rows="B"):
    """The packed table of mpc_set_instance_bounds_dev on the host: float64 (B, 12), a row being bu_lo[2], bu_hi[2], bx_lo[4], bx_hi[4] (bx in the
    order of mpc_config: x, y, v, omega).  Each group is (B, cols) or one row (cols,) for every instance; None takes cfg's value (an MpcConfig).
    `rows` is the caller's word for B in a shape message."""
    B = int(B)
    given = dict(bx_lo=bx_lo, bx_hi=bx_hi, bu_lo=bu_lo, bu_hi=bu_hi)
    tab = np.empty((B, BOUNDS_COLS))
    for name, at, cols in BOUNDS_ROW:
        a = given[name]
        tab[:, at:at + cols] = _bounds_group(name, list(getattr(cfg, name)) if a is None else a, cols, B, rows)
    return tab


class BatchedMpc:
    # lanes per horizon stage / wavefronts per SIMD / lanes per instance applied to every new handle (0 = automatic); test / tuning hooks,
    # also settable from the environment for profiling runs of unmodified programs (MPC_LANES_PER_STAGE, MPC_WAVES_PER_SIMD, MPC_LANES_PER_INSTANCE)
    default_lanes_per_stage = int(os.environ.get("MPC_LANES_PER_STAGE", "0"))
    default_waves_per_simd = int(os.environ.get("MPC_WAVES_PER_SIMD", "0"))
    default_lanes_per_instance = int(os.environ.get("MPC_LANES_PER_INSTANCE", "0"))
    default_block_riccati = int(os.environ.get("MPC_BLOCK_RICCATI", "0"))      # 1: stage recursions on pairs of stages (A/B runs of unmodified programs)
    default_matrix_cores = int(os.environ.get("MPC_MATRIX_CORES", "0"))      # 1: the v_mfma_f64_16x16x4 Riccati sweep (evidence path, one instance per wavefront)

    def __init__(self, N=20, n_obst=3, Tf=2.0, max_batch=1, device=0, **cfg_overrides):
        self.cfg = _lib.default_config(N, n_obst, Tf, **cfg_overrides)
        self.N, self.n_obst, self.Tf = int(N), int(n_obst), float(Tf)
        self.dt = self.Tf / self.N
        self.max_batch = int(max_batch)
        self.device = int(device)
        self._h = C.c_void_p()
        self._sqp_on, self._sqp_out, self._sqp_own = False, None, None      # set_sqp / set_sqp_iters_out
        _lib.check(_lib.lib().mpc_create2(C.byref(self.cfg), self.device, self.max_batch, C.byref(self._h)))
        if BatchedMpc.default_lanes_per_stage:
            _lib.check(_lib.lib().mpc_set_lanes_per_stage(self._h, int(BatchedMpc.default_lanes_per_stage)))
        if BatchedMpc.default_waves_per_simd:
            _lib.check(_lib.lib().mpc_set_waves_per_simd(self._h, int(BatchedMpc.default_waves_per_simd)))
        if BatchedMpc.default_lanes_per_instance:
            _lib.check(_lib.lib().mpc_set_lanes_per_instance(self._h, int(BatchedMpc.default_lanes_per_instance)))
        if BatchedMpc.default_block_riccati:
            _lib.check(_lib.lib().mpc_set_block_riccati(self._h, 1))
        if BatchedMpc.default_matrix_cores:
            _lib.check(_lib.lib().mpc_set_lanes_per_stage(self._h, 1))
            _lib.check(_lib.lib().mpc_set_lanes_per_instance(self._h, 64))
            _lib.check(_lib.lib().mpc_set_matrix_cores(self._h, 1))

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().mpc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------ host-pointer API (numpy in / numpy out)
    def reset_guess(self, x0):
        """set_initial_guess(), robot_ocp_problem.py:286-306."""
        x0 = _f64(np.atleast_2d(x0))
        _lib.check(_lib.lib().mpc_reset_guess(self._h, x0.shape[0], _ptr(x0)))

    def reset_guess_interp(self, x0, goal):
        """set_initial_guess() of the commented block :293-300 (the `interpolate_init` tables): straight line in y towards the goal."""
        x0 = _f64(np.atleast_2d(x0)); goal = _f64(np.atleast_2d(goal), (x0.shape[0], 2))
        _lib.check(_lib.lib().mpc_reset_guess_interp(self._h, x0.shape[0], _ptr(x0), _ptr(goal)))

    def set_warmstart(self, X, U):
        X, U = _f64(X), _f64(U)
        B = X.shape[0]
        if X.shape != (B, self.N + 1, 5) or U.shape != (B, self.N, 2):
            raise ValueError("X must be (B,N+1,5) and U (B,N,2)")
        _lib.check(_lib.lib().mpc_set_warmstart(self._h, B, _ptr(X), _ptr(U)))

    def get_traj(self, batch):
        X = np.empty((batch, self.N + 1, 5)); U = np.empty((batch, self.N, 2))
        _lib.check(_lib.lib().mpc_get_traj(self._h, batch, _ptr(X), _ptr(U)))
        return X, U

    def shift(self, batch):
        """warm-start shift, robot_ocp_problem.py:253-258."""
        _lib.check(_lib.lib().mpc_shift(self._h, batch))

    def solve(self, x0, obstacles, goal):
        """One RTI step for a batch.  `obstacles` is either the explicit parameter tensor P (B,N+1,n_obst,2)
        (reference API, parameterize_model) or obstacle states (B,n_obst,4) = (x,y,vx,vy) whose look-ahead is
        computed on the device.  Returns dict(u0, cost, status, iters); with set_sqp on also sqp_iters, the SQP iterations each instance ran."""
        x0 = _f64(np.atleast_2d(x0)); B = x0.shape[0]
        goal = _f64(np.atleast_2d(goal), (B, 2))
        obstacles = _f64(obstacles)
        u0 = np.empty((B, 2)); cost = np.empty(B)
        status = np.empty(B, np.int32); iters = np.empty(B, np.int32)
        if obstacles.shape == (B, self.N + 1, self.n_obst, 2):
            fn = _lib.lib().mpc_solve
        elif obstacles.shape == (B, self.n_obst, 4):
            fn = _lib.lib().mpc_solve_obst
        else:
            raise ValueError(f"obstacles must be (B,{self.N + 1},{self.n_obst},2) or (B,{self.n_obst},4), got {obstacles.shape}")
        if self._sqp_on and self._sqp_out is None:      # words of the handle's own, so that the count can be returned
            import torch
            self._sqp_own = torch.zeros(self.max_batch, dtype=torch.int32, device=torch.device("cuda", self.device))
            torch.cuda.synchronize(self.device)
            self.set_sqp_iters_out(self._sqp_own)
        _lib.check(fn(self._h, B, _ptr(x0), _ptr(obstacles), _ptr(goal), _ptr(u0), _ptr(cost), _ptr(status), _ptr(iters)))
        res = dict(u0=u0, cost=cost, status=status, iters=iters)
        if self._sqp_on:
            res["sqp_iters"] = self._sqp_out[:B].cpu().numpy().astype(np.int32)
        return res

    def set_sqp(self, max_iter=1, step_tol=0.0):
        """Several SQP iterations per solve launch (include/mpc_gpu.h mpc_set_sqp; acados' nlp_solver_type 'SQP' with nlp_solver_max_iter): every following
        solve, solve_dev and closed_loop_step_dev runs up to max_iter (2 .. 100) RTI iterations per instance on the launch's inputs, and an instance stops
        behind the iteration whose applied step has max-norm <= step_tol (0: never, inf: behind the first) or whose status is 4.  max_iter = 1: off."""
        _lib.check(_lib.lib().mpc_set_sqp(self._h, int(max_iter), float(step_tol)))
        self._sqp_on = int(max_iter) > 1

    def set_sqp_iters_out(self, out=None):
        """a contiguous int32 device tensor (max_batch,) that receives the SQP iterations each instance ran at every following solve (the word of an
        idle instance of the fused step is not written); None: off"""
        _check_device(f"the SQP iteration counts need a contiguous int32 device tensor ({self.max_batch},)", out, (self.max_batch,), ("torch.int32",))
        _lib.check(_lib.lib().mpc_set_sqp_iters_out_dev(self._h, _ptr(out)))
        self._sqp_out = out
        if out is not self._sqp_own:
            self._sqp_own = None

    def set_slack_schedule(self, alpha):
        """parameterize_slack(), robot_ocp_problem.py:145-152: explicit zl_i = Zl_i = alpha[b, i] for the following solves
        (alpha (B, N+1), or a device tensor of shape (max_batch, N+1) used in place); None = the reference's schedule, in-kernel."""
        if _is_host(alpha):
            alpha = _f64(np.atleast_2d(alpha))
            if alpha.shape[1] != self.N + 1:
                raise ValueError(f"alpha must be (B, {self.N + 1})")
            _lib.check(_lib.lib().mpc_set_slack_schedule(self._h, alpha.shape[0], _ptr(alpha)))
        else:      # a device tensor, or None (the library's one off path)
            _check_device(f"a device schedule must be ({self.max_batch}, {self.N + 1})", alpha, (self.max_batch, self.N + 1), contiguous=False)
            _lib.check(_lib.lib().mpc_set_slack_schedule_dev(self._h, _ptr(alpha)))

    def set_reference(self, yref, offset=None):
        """Per-stage reference, acados cost_set(stage, 'yref', v) (include/mpc_gpu.h mpc_set_reference): stage i of instance b tracks
        yref[b, min(offset[b] + i, T - 1)] in y order (x, y, v, omega, u_a, u_alpha); the terminal stage columns 0..3 of row min(offset[b] + N, T - 1).
        yref: a numpy array (B, T, 6) -- (B, N+1, 6) is a plain per-solve reference -- with an optional offset array (B,) (int32, copied), or a
        device tensor (max_batch, T, 6) used in place with an optional int32 device tensor (max_batch,) of offsets.  None clears it."""
        if yref is None:
            _lib.check(_lib.lib().mpc_set_reference(self._h, 0, 0, None, None))
        elif _is_host(yref):
            yref = _f64(yref)
            if yref.ndim != 3 or yref.shape[2] != 6:
                raise ValueError(f"yref must be (B, T, 6), got {yref.shape}")
            off = None
            if offset is not None:
                off = np.ascontiguousarray(offset, dtype=np.int32)
                if off.shape != (yref.shape[0],):
                    raise ValueError(f"offset must be ({yref.shape[0]},), got {off.shape}")
            _lib.check(_lib.lib().mpc_set_reference(self._h, yref.shape[0], yref.shape[1], _ptr(yref), _ptr(off)))
        else:
            _check_device(f"a device reference must be a contiguous ({self.max_batch}, T, 6) tensor", yref, (self.max_batch, None, 6))
            _check_device(f"device offsets must be a contiguous int32 tensor ({self.max_batch},)", offset, (self.max_batch,), ("torch.int32",))
            _lib.check(_lib.lib().mpc_set_reference_dev(self._h, int(yref.shape[1]), _ptr(yref), _ptr(offset)))

    def _instance_arrays(self, W, We, r_safe, r_hit):
        """host arrays of set_instance_params in the C layout: (B, 6), (B, 4), (B, n_obst), (B, n_obst); r_safe / r_hit of shape (B,) mean one radius
        per instance (every obstacle of it); all of one batch size.  None stays None."""
        out, B = [], None
        for (name, cols), a in zip(INSTANCE_ROW, (W, We, r_safe, r_hit)):
            if a is not None:
                a = instance_rows(name, a, cols, self.n_obst)
                if B is not None and a.shape[0] != B:
                    raise ValueError(f"{name} has {a.shape[0]} rows, the arrays before it {B}")
                B = a.shape[0]
            out.append(a)
        return out, B

    def set_instance_params(self, W=None, We=None, r_safe=None, r_hit=None):
        """Per-instance cost weights and per-obstacle radii (include/mpc_gpu.h mpc_set_instance_params): instance b solves with W[b] (6,) and We[b] (4,)
        in the order of mpc_config.W / .We, obstacle j of it with the safety radius r_safe[b, j] and, in the fused step's bookkeeping, the hit radius
        r_hit[b, j] (default r_safe[b, j] - (cfg.r_safe - 1.2)).  A group left None keeps the handle's value; all None switches the feature off.
        numpy arrays (B, 6), (B, 4), (B, n_obst) -- r_safe and r_hit also (B,), one radius per instance -- are validated and copied; device tensors
        (max_batch, ...) of exactly the C shapes are used in place (the values they hold when a solve is launched).  Not both kinds in one call."""
        host = {_is_host(a) for a in (W, We, r_safe, r_hit) if a is not None}
        if host == {True}:
            (W, We, r_safe, r_hit), B = self._instance_arrays(W, We, r_safe, r_hit)
            _lib.check(_lib.lib().mpc_set_instance_params(self._h, B, _ptr(W), _ptr(We), _ptr(r_safe), _ptr(r_hit)))
        elif True not in host:      # device tensors, or nothing given (the library's one off path)
            for name, a, cols in (("W", W, 6), ("We", We, 4), ("r_safe", r_safe, self.n_obst), ("r_hit", r_hit, self.n_obst)):
                _check_device(f"a device {name} must be a contiguous float64 tensor ({self.max_batch}, {cols})", a, (self.max_batch, cols), ("torch.float64",))
            _lib.check(_lib.lib().mpc_set_instance_params_dev(self._h, _ptr(W), _ptr(We), _ptr(r_safe), _ptr(r_hit)))
        else:
            raise ValueError("per-instance parameters: host arrays or device tensors, not both in one call")

    def set_obstacle_mask(self, active=None):
        """Per-instance obstacle masks (include/mpc_gpu.h mpc_set_obstacle_mask): active[b, j] says whether obstacle j exists for instance b.  An absent
        obstacle has no rows at any stage, no penalty in the reported cost and (unless STEP_MARGIN_ALL) no part in the fused step's margin; its entries
        in P / obst may hold anything.  A bool array (B, n_obst) is packed (pack_obstacle_mask), validated and copied; a device tensor (max_batch,) of
        int32 / uint32 words is used in place (the words it holds when a solve is launched; rewrite them on the device at will); None switches off."""
        if _is_host(active):
            a = mask_rows(active, self.n_obst)
            if a.shape[0] < 1 or a.shape[0] > self.max_batch:
                raise ValueError(f"active has {a.shape[0]} rows, the handle holds 1 .. {self.max_batch} instances")
            words = pack_obstacle_mask(a)
            _lib.check(_lib.lib().mpc_set_obstacle_mask(self._h, int(words.shape[0]), _ptr(words)))
        else:      # a device tensor, or None (the library's one off path)
            _check_device(f"a device obstacle mask must be a contiguous int32 / uint32 tensor ({self.max_batch},)", active, (self.max_batch,), ("torch.int32", "torch.uint32"))
            _lib.check(_lib.lib().mpc_set_obstacle_mask_dev(self._h, _ptr(active)))

    def set_instance_bounds(self, bx_lo=None, bx_hi=None, bu_lo=None, bu_hi=None):
        """Per-instance box bounds (include/mpc_gpu.h mpc_set_instance_bounds): instance b solves with the state box bx_lo[b] .. bx_hi[b] (4,) in the order
        of mpc_config (x, y, v, omega) and the input box bu_lo[b] .. bu_hi[b] (2,).  numpy arrays (B, 4) / (B, 2), validated and copied; a single row
        (4,) / (2,) is broadcast to the batch (max_batch when no group has rows of its own).  A group left None keeps the handle's value; all None
        switches the feature off."""
        given = dict(bx_lo=bx_lo, bx_hi=bx_hi, bu_lo=bu_lo, bu_hi=bu_hi)
        if all(a is None for a in given.values()):
            _lib.check(_lib.lib().mpc_set_instance_bounds(self._h, 0, None, None, None, None))
            return
        cols = {name: c for name, _, c in BOUNDS_ROW}
        rows = [np.asarray(a).shape[0] for a in given.values() if a is not None and np.asarray(a).ndim == 2]
        B = rows[0] if rows else self.max_batch
        arr = {name: (None if a is None else _bounds_group(name, a, cols[name], B)) for name, a in given.items()}
        _lib.check(_lib.lib().mpc_set_instance_bounds(self._h, int(B), _ptr(arr["bx_lo"]), _ptr(arr["bx_hi"]), _ptr(arr["bu_lo"]), _ptr(arr["bu_hi"])))

    def set_instance_bounds_dev(self, table):
        """The packed device form (mpc_set_instance_bounds_dev): a contiguous float64 device tensor (max_batch, 12) in the layout of pack_instance_bounds,
        used in place and not validated (the values it holds when a solve is launched; rewrite them on the device at will); None switches off."""
        _check_device(f"a device bounds table must be a contiguous float64 tensor ({self.max_batch}, {BOUNDS_COLS})", table, (self.max_batch, BOUNDS_COLS), ("torch.float64",))
        _lib.check(_lib.lib().mpc_set_instance_bounds_dev(self._h, _ptr(table)))

    def plant_step(self, x, u):
        """ocp_integrator set/solve/get, robot_ocp_problem.py:207-212."""
        x = _f64(np.atleast_2d(x)); u = _f64(np.atleast_2d(u), (x.shape[0], 2))
        xn = np.empty_like(x)
        _lib.check(_lib.lib().mpc_plant_step(self._h, x.shape[0], _ptr(x), _ptr(u), _ptr(xn)))
        return xn

    def predict(self, obst):
        """Obstacle.predict_trajectory for every obstacle -> P (B,N+1,n_obst,2), visualization.py:62-79."""
        obst = _f64(obst); B = obst.shape[0]
        if obst.shape != (B, self.n_obst, 4):
            raise ValueError("obst must be (B,n_obst,4)")
        P = np.empty((B, self.N + 1, self.n_obst, 2))
        _lib.check(_lib.lib().mpc_predict(self._h, B, _ptr(obst), _ptr(P)))
        return P

    SCENARIOS = {"RANDOM": 0, "CENTER": 1, "EDGE": 2}

    @staticmethod
    def _scenario_box():
        from . import world as w
        return np.array([w.X_MIN_OBST, w.X_MAX_OBST, w.Y_MIN_OBST, w.Y_MAX_OBST, w.V_MAX_OBST, 7.0], dtype=np.float64)

    def generate_scenarios(self, scenario, count, seed0=0):
        """generate_random_moving_obstacles for np.random.seed(seed0 + s), s < count (obstacle_generator.py:8-28) -> (count, n_obst, 4)"""
        obst = np.empty((count, self.n_obst, 4))
        box = self._scenario_box()
        _lib.check(_lib.lib().mpc_generate_scenarios(self._h, count, self.SCENARIOS[scenario], seed0, _ptr(box), _ptr(obst)))
        return obst

    def generate_scenarios_dev(self, scenario, count, obst, seed0=0, stream=None):
        box = self._scenario_box()
        _lib.check(_lib.lib().mpc_generate_scenarios_dev(self._h, count, self.SCENARIOS[scenario], seed0, _ptr(box), _ptr(obst), _ptr(stream)))

    def noise_state(self, count, scenario, seed0=0, stream=None):
        """device generator states of `count` instances after np.random.seed(seed0 + s) and the scenario draw (a torch int32 tensor)"""
        import torch
        st = torch.zeros(count, _lib.lib().mpc_noise_state_words(), dtype=torch.int32, device=torch.device("cuda", self.device))
        _lib.check(_lib.lib().mpc_noise_init_dev(self._h, count, self.SCENARIOS[scenario], seed0, _ptr(st), _ptr(stream)))
        return st

    def noise_draw_dev(self, count, state, noise, ep_flags=None, stream=None):
        """one control step's normals of the reference's stream -> noise (count, n_obst, 2); advances `state`"""
        _lib.check(_lib.lib().mpc_noise_draw_dev(self._h, count, _ptr(state), _ptr(noise), _ptr(ep_flags), _ptr(stream)))

    def episode_refill_dev(self, slots, scenario, seed_first, seed_count, max_steps, start, goal_rows, per_seed, x0, obst, goal, X, U, min_margin,
                           ep_flags, ep_steps, state, noise, slot_seed, cursor, res_f, res_i, flags=0, stream=None):
        """one refill of a seed sweep, in front of closed_loop_step_dev (include/mpc_gpu.h mpc_episode_refill_dev): finished slots park their result
        rows under their seed index and start the next seed indices in ascending slot order; flags: OR of _lib.REFILL_*"""
        box = self._scenario_box()
        _lib.check(_lib.lib().mpc_episode_refill_dev(self._h, int(slots), self.SCENARIOS[scenario], int(seed_first), int(seed_count), int(max_steps), int(flags),
                                                     _ptr(box), _ptr(start), _ptr(goal_rows), 1 if per_seed else 0, _ptr(x0), _ptr(obst), _ptr(goal), _ptr(X),
                                                     _ptr(U), _ptr(min_margin), _ptr(ep_flags), _ptr(ep_steps), _ptr(state), _ptr(noise), _ptr(slot_seed),
                                                     _ptr(cursor), _ptr(res_f), _ptr(res_i), _ptr(stream)))

    def set_refill_tables_dev(self, W=None, We=None, r_safe=None, r_hit=None, mask=None, bounds=None, slot_W=None, slot_We=None, slot_r_safe=None,
                              slot_r_hit=None, slot_mask=None, slot_bounds=None, log=None, res_log=None):
        """Per-seed tables and the status log of a sweep (include/mpc_gpu.h mpc_set_refill_tables_dev), device tensors used in place: when seed index k
        starts in slot s, episode_refill_dev copies row k of every source given (W (count, 6), We (count, 4), r_safe / r_hit (count, n_obst), mask (count,)
        int32 words, bounds (count, 12)) into row s of its slot_ destination -- the per-slot tensor registered with set_instance_params /
        set_obstacle_mask / set_instance_bounds_dev -- resets log[s] (slots, 4) and parks it under the old seed in res_log (count, 3).  Nothing is validated
        here beyond source / destination pairing (the library's); all None switches off."""
        given = dict(W=W, We=We, r_safe=r_safe, r_hit=r_hit, mask=mask, bounds=bounds, slot_W=slot_W, slot_We=slot_We, slot_r_safe=slot_r_safe,
                     slot_r_hit=slot_r_hit, slot_mask=slot_mask, slot_bounds=slot_bounds, log=log, res_log=res_log)
        if all(a is None for a in given.values()):
            _lib.check(_lib.lib().mpc_set_refill_tables_dev(self._h, None))
            return
        t = _lib.RefillTables(**{n: _ptr(a) for n, a in given.items()})
        _lib.check(_lib.lib().mpc_set_refill_tables_dev(self._h, C.byref(t)))

    def episode_status_log_dev(self, slots, status, ep_flags, ep_steps, log, stream=None):
        """behind closed_loop_step_dev on the same stream: counts the step's status words into log (slots, 4) = n2, n4, first_bad, seen per slot
        (include/mpc_gpu.h mpc_episode_status_log_dev)"""
        _lib.check(_lib.lib().mpc_episode_status_log_dev(self._h, int(slots), _ptr(status), _ptr(ep_flags), _ptr(ep_steps), _ptr(log), _ptr(stream)))

    def episode_ring_dev(self, capacity, ring_state=None, ring_obst=None, ring_tag=None, seed_src=None):
        """attach a ring of `capacity` seeded episodes to the refill (include/mpc_gpu.h mpc_episode_ring_dev): ring_state (capacity, noise state words) int32,
        ring_obst (capacity, n_obst, 4), ring_tag (capacity,) int32 preset to -1, seed_src (count,) int32 or None; capacity 0 detaches"""
        _lib.check(_lib.lib().mpc_episode_ring_dev(self._h, int(capacity), _ptr(ring_state), _ptr(ring_obst), _ptr(ring_tag), _ptr(seed_src)))

    def episode_ring_fill_dev(self, scenario, seed_first, seed_count, cursor, stream=None):
        """one fill of the attached ring, in front of episode_refill_dev on the same stream: seeds the entries of the next `capacity` seed indices behind
        cursor[0] that the ring does not hold yet (include/mpc_gpu.h mpc_episode_ring_fill_dev)"""
        box = self._scenario_box()
        _lib.check(_lib.lib().mpc_episode_ring_fill_dev(self._h, self.SCENARIOS[scenario], int(seed_first), int(seed_count), _ptr(box), _ptr(cursor), _ptr(stream)))

    TRACE_FIELDS = ("seed_row", "slot_state", "len", "x", "obst", "u", "status", "iters", "pred")

    def episode_trace_set_dev(self, rows=0, max_steps=0, seed_row=None, slot_state=None, len=None, x=None, obst=None, u=None, status=None, iters=None, pred=None):
        """attach the per-seed trajectory arrays of a sweep (include/mpc_gpu.h mpc_episode_trace_set_dev), device tensors used in place: seed_row (count,) int32
        = the row of each seed index or -1 (the non-negative entries distinct: the caller's to guarantee), slot_state (slots, 2) int32 preset {-1, 0}, len (rows,)
        int32, x (rows, max_steps + 1, 5), obst (rows, max_steps + 1, n_obst, 4), u (rows, max_steps, 2), status / iters (rows, max_steps) int32, pred
        (rows, max_steps, N + 1, 5) or None.  rows 0 (the default) detaches.  trace_shapes keeps the shapes of the arrays last attached."""
        given = dict(seed_row=seed_row, slot_state=slot_state, len=len, x=x, obst=obst, u=u, status=status, iters=iters, pred=pred)
        if int(rows) == 0:
            _lib.check(_lib.lib().mpc_episode_trace_set_dev(self._h, 0, 0, None))
            return
        t = _lib.EpisodeTrace(**{n: _ptr(a) for n, a in given.items()})
        _lib.check(_lib.lib().mpc_episode_trace_set_dev(self._h, int(rows), int(max_steps), C.byref(t)))
        self.trace_shapes = {n: tuple(a.shape) for n, a in given.items() if hasattr(a, "shape")}

    def episode_trace_dev(self, slots, phase, slot_seed, x0, obst, X=None, u0=None, status=None, iters=None, ep_flags=None, ep_steps=None, stream=None):
        """one launch of the attached trace (include/mpc_gpu.h mpc_episode_trace_dev): phase _lib.TRACE_START behind episode_refill_dev, _lib.TRACE_STEP behind
        closed_loop_step_dev (which then takes a u0 array) and episode_status_log_dev, all on one stream"""
        _lib.check(_lib.lib().mpc_episode_trace_dev(self._h, int(slots), int(phase), _ptr(slot_seed), _ptr(x0), _ptr(obst), _ptr(X), _ptr(u0), _ptr(status),
                                                    _ptr(iters), _ptr(ep_flags), _ptr(ep_steps), _ptr(stream)))

    GROUP_RECORD_FIELDS = ("group_row", "len", "x", "obst", "u", "winner", "best_key", "cand_key", "cand_status", "cand_iters", "cand_u0", "cand_X")

    def group_record_set_dev(self, rows=0, max_steps=0, K=0, group_row=None, len=None, x=None, obst=None, u=None, winner=None, best_key=None, cand_key=None,
                             cand_status=None, cand_iters=None, cand_u0=None, cand_X=None):
        """attach the per-group record of multi-start episodes (include/mpc_gpu.h mpc_group_record_set_dev), device tensors used in place: group_row (groups,)
        int32 = the row of each group or -1 (the non-negative entries distinct: the caller's to guarantee), len (rows,) int32 preset 0, x (rows, max_steps + 1, 5),
        obst (rows, max_steps + 1, n_obst, 4), u (rows, max_steps, 2), winner (rows, max_steps) int32, best_key (rows, max_steps), cand_key (rows, max_steps, K),
        cand_status / cand_iters (rows, max_steps, K) int32, cand_u0 (rows, max_steps, K, 2), cand_X (rows, max_steps, K, N + 1, 5) or None.  rows 0 (the default)
        detaches.  group_record_shapes keeps the shapes of the arrays last attached."""
        given = dict(group_row=group_row, len=len, x=x, obst=obst, u=u, winner=winner, best_key=best_key, cand_key=cand_key, cand_status=cand_status,
                     cand_iters=cand_iters, cand_u0=cand_u0, cand_X=cand_X)
        if int(rows) == 0:
            _lib.check(_lib.lib().mpc_group_record_set_dev(self._h, 0, 0, 0, None))
            return
        r = _lib.GroupRecord(**{n: _ptr(a) for n, a in given.items()})
        _lib.check(_lib.lib().mpc_group_record_set_dev(self._h, int(rows), int(max_steps), int(K), C.byref(r)))
        self.group_record_shapes = {n: tuple(a.shape) for n, a in given.items() if hasattr(a, "shape")}

    def group_record_dev(self, groups, K, phase, x, obst, X, key, status, iters, u0, out, stream=None):
        """one launch of the attached group record (include/mpc_gpu.h mpc_group_record_dev): phase _lib.GROUP_RECORD_SOLVED behind the member solve (and the
        rollout merit) and in front of mpc_group_step_dev, _lib.GROUP_RECORD_STEPPED behind it, all on one stream; `out` is that call's _lib.GroupStepOut"""
        _lib.check(_lib.lib().mpc_group_record_dev(self._h, int(groups), int(K), int(phase), _ptr(x), _ptr(obst), _ptr(X), _ptr(key), _ptr(status), _ptr(iters),
                                                   _ptr(u0), None if out is None else C.byref(out), _ptr(stream)))

    # ------------------------------------------------------------------ multi-GPU: all-gather of the costs, RCCL called by the library itself
    @staticmethod
    def comm_unique_id():
        """128 bytes that rank 0 creates and hands to every rank (any transport: a file, a socket, torch.distributed's store)"""
        buf = (C.c_ubyte * _lib.COMM_ID_BYTES)()
        _lib.check(_lib.lib().mpc_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, rank, world, unique_id):
        """collective: this handle becomes rank `rank` of `world` of the cost exchange"""
        if len(unique_id) != _lib.COMM_ID_BYTES:
            raise ValueError(f"unique_id must be {_lib.COMM_ID_BYTES} bytes")
        buf = (C.c_ubyte * _lib.COMM_ID_BYTES).from_buffer_copy(unique_id)
        _lib.check(_lib.lib().mpc_comm_init(self._h, int(rank), int(world), buf))

    def comm_world(self):
        return int(_lib.lib().mpc_comm_world(self._h))

    def comm_destroy(self):
        _lib.check(_lib.lib().mpc_comm_destroy(self._h))

    @staticmethod
    def comm_library_path():
        """file name of the RCCL library the exchange is bound to (mpc_comm_library_path)"""
        buf = C.create_string_buffer(1024)
        _lib.check(_lib.lib().mpc_comm_library_path(buf, len(buf)))
        return buf.value.decode()

    def allgather_cost_dev(self, count, cost, cost_all, stream=None):
        """collective: cost (count,) of every rank -> cost_all (world, count), rank-major; device arrays, enqueued on `stream`"""
        _lib.check(_lib.lib().mpc_allgather_cost_dev(self._h, int(count), _ptr(cost), _ptr(cost_all), _ptr(stream)))

    def allgather_cost(self, cost):
        """collective, host arrays: returns (world, count)"""
        cost = _f64(cost).ravel()
        out = np.empty((self.comm_world(), cost.size))
        _lib.check(_lib.lib().mpc_allgather_cost(self._h, int(cost.size), _ptr(cost), _ptr(out)))
        return out

    def terminal_state(self, batch):
        """x_N of the current iterate (the reference reads it at robot_ocp_problem.py:232; hook for a sub-goal policy)"""
        return self.get_traj(batch)[0][:, -1].copy()

    # ------------------------------------------------------------------ device-pointer API (torch tensors or raw ints)
    def iterate_ptrs(self):
        dX, dU, st = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.check(_lib.lib().mpc_iterate_ptrs(self._h, C.byref(dX), C.byref(dU), C.byref(st)))
        return dX.value, dU.value, st.value

    def solve_dev(self, batch, x0, P, goal, X, U, u0=None, cost=None, status=None, iters=None, stream=None):
        _lib.check(_lib.lib().mpc_solve_dev(self._h, batch, _ptr(x0), _ptr(P), _ptr(goal), _ptr(X), _ptr(U), _ptr(u0),
                                            _ptr(cost), _ptr(status), _ptr(iters), _ptr(stream)))

    def closed_loop_step_dev(self, batch, x0, obst, goal, X, U, u0=None, cost=None, status=None, iters=None, noise=None,
                             randomness=0.1, vmax=2.0, flags=_lib.STEP_SHIFT | _lib.STEP_PLANT | _lib.STEP_OBSTACLES,
                             min_margin=None, ep_flags=None, ep_steps=None, stream=None):
        """One whole control step (look-ahead, solve, plant, obstacle motion, bookkeeping, shift) in one launch.  flags | STEP_MARGIN_ALL lets the margin and
        the hit flag count obstacles that set_obstacle_mask masks off; flags | STEP_ADVANCE_REF moves
        the per-stage reference window (set_reference with offsets) one row on for every instance that stepped."""
        _lib.check(_lib.lib().mpc_closed_loop_step_dev(self._h, batch, _ptr(x0), _ptr(obst), _ptr(goal), _ptr(X), _ptr(U), _ptr(u0),
                                                       _ptr(cost), _ptr(status), _ptr(iters), _ptr(noise), randomness, vmax, flags,
                                                       _ptr(min_margin), _ptr(ep_flags), _ptr(ep_steps), _ptr(stream)))

    def predict_dev(self, batch, obst, P, stream=None):
        _lib.check(_lib.lib().mpc_predict_dev(self._h, batch, _ptr(obst), _ptr(P), _ptr(stream)))

    def rollout_merit_dev(self, batch, x0, P, goal, U, X=None, merit=None, defect=None, margin=None, boxviol=None, Xr=None, members=1, stream=None):
        """Score the plans U (batch, N, 2) by simulating them (include/mpc_gpu.h mpc_rollout_merit_dev): X^r rolled out from x0 with the plant's integrator,
        merit (batch,) the NLP objective at (X^r, U) as the solve launched now would report it, defect (batch,) of the given iterate X (batch, N+1, 5),
        margin (batch,) of X^r to the obstacles, boxviol (batch,) of the state boxes by X^r, Xr (batch, N+1, 5).  Instance b reads row b // members of
        x0, P (rows, N+1, n_obst, 2) and goal.  Device tensors; every output is optional, at least one must be given, and defect needs X."""
        _lib.check(_lib.lib().mpc_rollout_merit_dev(self._h, int(batch), int(members), _ptr(x0), _ptr(P), _ptr(goal), _ptr(X), _ptr(U), _ptr(merit),
                                                    _ptr(defect), _ptr(margin), _ptr(boxviol), _ptr(Xr), _ptr(stream)))

    def shift_dev(self, batch, X, U, stream=None):
        _lib.check(_lib.lib().mpc_shift_dev(self._h, batch, _ptr(X), _ptr(U), _ptr(stream)))

    def reset_guess_dev(self, batch, x0, X, U, stream=None):
        _lib.check(_lib.lib().mpc_reset_guess_dev(self._h, batch, _ptr(x0), _ptr(X), _ptr(U), _ptr(stream)))

    def reset_guess_interp_dev(self, batch, x0, goal, X, U, stream=None):
        _lib.check(_lib.lib().mpc_reset_guess_interp_dev(self._h, batch, _ptr(x0), _ptr(goal), _ptr(X), _ptr(U), _ptr(stream)))

    def plant_step_dev(self, batch, x, u, xn, stream=None):
        _lib.check(_lib.lib().mpc_plant_step_dev(self._h, batch, _ptr(x), _ptr(u), _ptr(xn), _ptr(stream)))

    def obstacle_step_dev(self, count, obst, noise=None, randomness=0.1, vmax=2.0, stream=None):
        _lib.check(_lib.lib().mpc_obstacle_step_dev(self._h, count, _ptr(obst), _ptr(noise), randomness, vmax, _ptr(stream)))

    def linearize_dev(self, batch, x0, P, goal, X, U, A, B, b, q, hval, dh, stream=None):
        _lib.check(_lib.lib().mpc_linearize_dev(self._h, batch, _ptr(x0), _ptr(P), _ptr(goal), _ptr(X), _ptr(U), _ptr(A), _ptr(B),
                                                _ptr(b), _ptr(q), _ptr(hval), _ptr(dh), _ptr(stream)))

    def debug_adjoint_dev(self, batch, lanes_per_instance, lanes_per_stage, X, U, g, ru, stream=None):
        """the polish's stationarity sweep on its own (mpc_debug_adjoint_dev): ru[B][N] from a given gradient g[B][N+1][7] over the linearisation of (X, U)"""
        _lib.check(_lib.lib().mpc_debug_adjoint_dev(self._h, batch, int(lanes_per_instance), int(lanes_per_stage), _ptr(X), _ptr(U), _ptr(g), _ptr(ru), _ptr(stream)))

    # ------------------------------------------------------------------ measurement
    def set_accumulators(self, iters_acc=None, status_acc=None):
        _lib.check(_lib.lib().mpc_set_accumulators(self._h, _ptr(iters_acc), _ptr(status_acc)))

    def debug_trace(self, enable=True, batch=None):
        """(mu, sigma, alpha, cmax) of every interior-point iteration of the following solves (include/mpc_gpu.h mpc_debug_trace): switches the record
        on or off and returns what it held, (batch, qp_iter_max, 4) with instance b's iterations in block b -- zeros right after enabling and while
        it is off.  The call waits for the handle's stream only: a caller who solved on another stream synchronises that stream first."""
        batch = self.max_batch if batch is None else int(batch)
        out = np.zeros((batch if 1 <= batch <= self.max_batch else 1, int(self.cfg.qp_iter_max), 4))      # (`batch` itself is the library's to judge)
        _lib.check(_lib.lib().mpc_debug_trace(self._h, 1 if enable else 0, batch, _ptr(out)))
        return out

    def profile_enable(self, on=True, every=1):
        """HIP events around every `every`-th solve launch (on=False: off)."""
        _lib.check(_lib.lib().mpc_profile_enable(self._h, int(every) if on else 0))

    def profile_read(self):
        ms, n = C.c_double(), C.c_int()
        _lib.check(_lib.lib().mpc_profile_read(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def set_row_parallel(self, on=True):
        """Riccati factorisation sweep: row-parallel 64-bit-DPP variant (True) or one-lane systolic sweep (False)."""
        _lib.check(_lib.lib().mpc_set_row_parallel(self._h, 1 if on else 0))

    def set_block_riccati(self, on=True):
        """stage recursions over pairs of stages (opt-in) or one stage per step (default) (mpc_set_block_riccati)"""
        _lib.check(_lib.lib().mpc_set_block_riccati(self._h, 1 if on else 0))

    def set_matrix_cores(self, on=True):
        _lib.check(_lib.lib().mpc_set_matrix_cores(self._h, 1 if on else 0))

    def set_lanes_per_instance(self, lanes):
        _lib.check(_lib.lib().mpc_set_lanes_per_instance(self._h, int(lanes)))

    def lanes_per_instance(self, batch):
        return _lib.lib().mpc_get_lanes_per_instance(self._h, batch)

    def set_lanes_per_stage(self, lanes):
        """0 automatic (small batches: rows of a stage split over 2-3 lanes), 1 one lane per stage, 2 / 3 split mapping."""
        _lib.check(_lib.lib().mpc_set_lanes_per_stage(self._h, int(lanes)))

    def lanes_per_stage(self, batch):
        return _lib.lib().mpc_get_lanes_per_stage(self._h, batch)

    def kernel_name(self, batch, lookahead=True):
        """the solve kernel instantiation a batch of this size runs, as a profiler prints it (without the namespace)"""
        buf = C.create_string_buffer(96)
        _lib.check(_lib.lib().mpc_get_kernel_name(self._h, batch, 1 if lookahead else 0, buf, 96))
        return buf.value.decode()

    def set_instance_scheduling(self, on=True):
        """deal instances to wavefronts in the order of their previous iteration counts (mappings with several instances per wavefront)"""
        _lib.check(_lib.lib().mpc_set_instance_scheduling(self._h, 1 if on else 0))

    def instance_order(self, batch):
        """the permutation in effect for the next launch of `batch` instances, or None for the natural order"""
        order = np.empty(batch, np.int32)
        rc = _lib.lib().mpc_get_instance_order(self._h, batch, _ptr(order))
        if rc < 0:
            _lib.check(rc)
        return order if rc == 1 else None

    def set_waves_per_simd(self, waves):
        """stage-split mapping: 0 automatic, 1 one wavefront per SIMD (512 registers), 2 two (256 registers, compact LDS blocks)"""
        _lib.check(_lib.lib().mpc_set_waves_per_simd(self._h, int(waves)))

    def waves_per_simd(self, batch):
        return _lib.lib().mpc_get_waves_per_simd(self._h, batch)
