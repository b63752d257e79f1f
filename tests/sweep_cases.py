"""Shared constants and the small slot-array harness of the seed-sweep tests (test_sweep_host.py, test_gpu_sweep.py).

The problem is the reference's own (experiments.py:20-36): N 20, 5 obstacles, Tf 2, start [-7, -7, pi/4, 0, 0], goal [7, 7], QP_ITER 100.
`batch_reference` is the yardstick of the GPU tests: run_episodes on ONE batch holding every seed -- the path that exists without the sweep -- computed once
per (mapping, scenario, seeds, options) and shared."""
import numpy as np

START = np.array([-7.0, -7.0, np.pi / 4, 0.0, 0.0])
GOAL = np.array([7.0, 7.0])
PROBLEM = dict(N=20, Tf=2.0, n_obst=5, qp_iter_max=100)
WIDE_PROBLEM = dict(N=10, Tf=1.0, n_obst=15, qp_iter_max=100)        # more than ten obstacles: the multi-wavefront solve kernel, the full-state scenario draw
RECORDED = {"RANDOM": "20221031_215846", "EDGE": "20221031_220136"}      # the TF 2 / N 20 / QP_ITER 100 tables of tests/golden/reference_tables.json

# the arrays one refill call may write, in the order of the C prototype
SLOT_ARRAYS = ("x0", "obst", "goal", "X", "U", "margin", "flags", "steps", "state", "noise", "slot_seed")
ALL_ARRAYS = SLOT_ARRAYS + ("cursor", "res_f", "res_i")


def per_seed_rows(count, seed=11):
    """`count` distinct start and goal rows inside the arena, away from its walls"""
    rng = np.random.default_rng(seed)
    start = np.zeros((count, 5)); start[:, 0] = rng.uniform(-7.5, -5.5, count); start[:, 1] = rng.uniform(-7.5, -5.5, count)
    start[:, 2] = rng.uniform(0.2, 1.3, count); start[:, 3] = rng.uniform(0.0, 0.5, count); start[:, 4] = rng.uniform(-0.2, 0.2, count)
    goal = np.column_stack([rng.uniform(5.5, 7.5, count), rng.uniform(5.5, 7.5, count)])
    return start, goal


_REF = {}


def batch_reference(mpc_gpu, scenario, first, count, start=None, goal=None, problem=PROBLEM, **kw):
    """run_episodes(start, goal, scenario, first_seed=first) at B = count without compaction, on the lane mapping in effect; cached, returned read-only"""
    key = repr((mpc_gpu.BatchedMpc.default_lanes_per_stage, scenario, first, count, None if start is None else start.tobytes(),
                None if goal is None else goal.tobytes(), sorted(problem.items()), sorted(kw.items())))
    if key not in _REF:
        x0 = np.tile(START, (count, 1)) if start is None else start
        g = np.tile(GOAL, (count, 1)) if goal is None else goal
        r = mpc_gpu.run_episodes(x0, g, scenario, first_seed=first, compact_from=None, **problem, **kw)
        for a in (r["table"], r["x_last"]):
            a.setflags(write=False)
        _REF[key] = r
    return _REF[key]


class Plain:
    """the allocator interface of feature_loop.Banded without the bands"""

    def __init__(self, torch, dev):
        self.torch, self.dev = torch, dev

    def f64(self, *shape, init=0.0):
        return self.torch.full(shape, init, dtype=self.torch.float64, device=self.dev)

    def i32(self, *shape, init=0):
        return self.torch.full(shape, init, dtype=self.torch.int32, device=self.dev)


class SlotArrays:
    """every array of mpc_episode_refill_dev for `slots` slots and `count` seeds, preset as the first call of a sweep wants them"""

    def __init__(self, alloc, m, slots, count, words, per_seed_start=None, per_seed_goal=None):
        torch = alloc.torch
        N, no = m.N, m.n_obst
        self.slots, self.count = slots, count
        self.x0 = alloc.f64(slots, 5); self.obst = alloc.f64(slots, no, 4); self.goal = alloc.f64(slots, 2)
        self.X = alloc.f64(slots, N + 1, 5); self.U = alloc.f64(slots, N, 2)
        self.margin = alloc.f64(slots, init=float("inf"))
        self.flags = alloc.i32(slots, init=1); self.steps = alloc.i32(slots)
        self.state = alloc.i32(slots, words); self.noise = alloc.f64(slots, no, 2)
        self.slot_seed = alloc.i32(slots, init=-1); self.cursor = alloc.i32(2)
        self.res_f = alloc.f64(count, 6, init=float("nan")); self.res_i = alloc.i32(count, 2, init=-1)
        self.status = alloc.i32(slots); self.iters = alloc.i32(slots)
        self.per_seed = per_seed_start is not None
        s = np.atleast_2d(START if per_seed_start is None else per_seed_start); g = np.atleast_2d(GOAL if per_seed_goal is None else per_seed_goal)
        self.start_rows = alloc.f64(*s.shape); self.start_rows.copy_(torch.from_numpy(np.ascontiguousarray(s)))
        self.goal_rows = alloc.f64(*g.shape); self.goal_rows.copy_(torch.from_numpy(np.ascontiguousarray(g)))

    def snapshot(self, names=ALL_ARRAYS, rows=slice(None)):
        """host copies (the caller synchronises); `rows` selects slots of the per-slot arrays"""
        return {n: (getattr(self, n)[rows] if n in SLOT_ARRAYS else getattr(self, n)).cpu().numpy().copy() for n in names}

    def refill(self, m, scenario, first, max_steps, flags, stream, slots=None, count=None):
        m.episode_refill_dev(self.slots if slots is None else slots, scenario, first, self.count if count is None else count, max_steps, self.start_rows,
                             self.goal_rows, self.per_seed, self.x0, self.obst, self.goal, self.X, self.U, self.margin, self.flags, self.steps, self.state,
                             self.noise, self.slot_seed, self.cursor, self.res_f, self.res_i, flags=flags, stream=stream)

    def step(self, m, step_flags, stream):
        m.closed_loop_step_dev(self.slots, self.x0, self.obst, self.goal, self.X, self.U, None, None, self.status, self.iters, self.noise, flags=step_flags,
                               min_margin=self.margin, ep_flags=self.flags, ep_steps=self.steps, stream=stream)

    def table(self):
        """the rows as run_episodes forms them, from the parked raw words"""
        ri, rf = self.res_i.cpu().numpy(), self.res_f.cpu().numpy()
        goal = np.broadcast_to(self.goal_rows.cpu().numpy(), (self.count, 2))
        fl, xl = ri[:, 0], rf[:, 1:6]
        return np.column_stack([(fl & 4) != 0, (fl & 1) != 0, rf[:, 0], np.linalg.norm(xl[:, :2] - goal, axis=1), ri[:, 1], (fl & 2) != 0]).astype(np.float64), xl
