"""Shared cases of the per-seed sweep features (test_sweep_features_host.py, test_gpu_sweep_features.py): the per-seed arrays, drawn once from a fixed
generator, the yardstick -- run_episodes on ONE batch that holds every seed, given the same arrays per instance (sweep_cases.batch_reference with
features) -- and the device arrays of mpc_set_refill_tables_dev / mpc_episode_ring_dev for tests that drive the entry points themselves."""
import numpy as np

import sweep_cases as sc

HANDLE = dict(W=[2, 2, 2, 2, 0.15, 0.15], We=[5, 5, 5, 5], r_safe=2.4, r_hit=1.2, bu_hi=[8, 8], bx_hi=[7, 7, 10, 10])       # mpc_default_config


def arrays(count, n_obst=5, seed=3):
    """per-seed arrays for `count` seeds; row k is a function of (seed, k) only through the generator's order, so arrays(24)[:12] != arrays(12) -- slice"""
    rng = np.random.default_rng(seed)
    r_safe = rng.uniform(1.6, 2.6, (count, n_obst))
    r_hit = r_safe - rng.uniform(0.6, 1.3, (count, n_obst))
    active = rng.random((count, n_obst)) < 0.6
    active[np.arange(count), rng.integers(0, n_obst, count)] = True            # every seed keeps an obstacle ...
    active[np.arange(count), (np.argmax(active, axis=1) + 1) % n_obst] = False  # ... and loses one
    W = np.column_stack([rng.uniform(1.0, 3.0, (count, 4)), rng.uniform(0.05, 0.3, (count, 2))])
    We = rng.uniform(3.0, 8.0, (count, 4))
    bu_hi = rng.uniform(1.5, 5.0, (count, 2))
    bx_hi = np.column_stack([np.full((count, 2), 7.0), rng.uniform(1.2, 3.0, count), rng.uniform(2.0, 6.0, count)])
    a = dict(r_safe=r_safe, r_hit=r_hit, active=active, W=W, We=We, bounds=dict(bu_lo=-bu_hi, bu_hi=bu_hi, bx_hi=bx_hi))      # bx_lo: the handle's
    # at least one seed differs from the handle's value in every table
    assert (r_safe != HANDLE["r_safe"]).any() and (r_hit != HANDLE["r_hit"]).any() and (~active).any()
    assert (W != HANDLE["W"]).any() and (We != HANDLE["We"]).any() and (bu_hi != HANDLE["bu_hi"]).any() and (bx_hi != HANDLE["bx_hi"]).any()
    return a


# feature set -> the names of arrays() it uses (and margin_all)
FEATURES = {
    "radii": ("r_safe",),
    "radii-and-hit": ("r_safe", "r_hit"),
    "mask": ("active",),
    "mask-margin-all": ("active", "margin_all"),
    "bounds": ("bounds",),
    "weights": ("W", "We"),
    "all": ("r_safe", "r_hit", "active", "margin_all", "bounds", "W", "We"),
}


def feature_kwargs(name, count, rows=slice(None), total=None):
    """run_seed_sweep's keyword arguments of a feature set: rows `rows` of arrays(total or count)"""
    a = arrays(count if total is None else total)
    out = {}
    for n in FEATURES[name]:
        if n == "margin_all":
            out[n] = True
        elif n == "bounds":
            out[n] = {k: v[rows] for k, v in a[n].items()}
        else:
            out[n] = a[n][rows]
    return out


_REF = {}


def batch_feature_reference(mpc_gpu, scenario, first, count, name, problem=sc.PROBLEM, **kw):
    """the yardstick: run_episodes at B = count without compaction, given feature set `name` per instance.  Cost weights go through the handle
    (set_instance_params, with the radii when both are set: run_episodes' own r_safe / r_hit would replace the handle's weights); cached, read-only"""
    key = repr((mpc_gpu.BatchedMpc.default_lanes_per_stage, scenario, first, count, name, sorted(problem.items()), sorted(kw.items())))
    if key not in _REF:
        f = feature_kwargs(name, count)
        x0, g = np.tile(sc.START, (count, 1)), np.tile(sc.GOAL, (count, 1))
        if "W" in f:
            with mpc_gpu.BatchedMpc(max_batch=count, **problem) as m:
                m.set_instance_params(W=f.pop("W"), We=f.pop("We"), r_safe=f.pop("r_safe", None), r_hit=f.pop("r_hit", None))
                r = mpc_gpu.run_episodes(x0, g, scenario, first_seed=first, compact_from=None, solver=m, N=problem["N"], Tf=problem["Tf"],
                                         n_obst=problem["n_obst"], **f, **kw)
        else:
            r = mpc_gpu.run_episodes(x0, g, scenario, first_seed=first, compact_from=None, **problem, **f, **kw)
        for a in (r["table"], r["x_last"]):
            a.setflags(write=False)
        _REF[key] = r
    return _REF[key]


TABLE_ARRAYS = ("slot_W", "slot_We", "slot_r_safe", "slot_r_hit", "slot_mask", "slot_bounds", "log")
RING_ARRAYS = ("ring_state", "ring_obst", "ring_tag")


class FeatureArrays:
    """the device arrays of the "all" feature set for a handle of `rows` = max_batch instances and `count` seeds, preset as run_seed_sweep presets them and
    registered on the handle: per-seed sources, per-slot destinations, log / res_log, and (capacity given) a ring with its seed_src"""

    def __init__(self, alloc, m, count, capacity=None, total=None):
        import mpc_gpu.solver as sv
        torch = alloc.torch
        rows, no = m.max_batch, m.n_obst
        f = feature_kwargs("all", count, slice(0, count), total=total)
        put = lambda dst, a: dst.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        src = dict(W=f["W"], We=f["We"], r_safe=f["r_safe"], r_hit=f["r_hit"])
        preset = dict(W=HANDLE["W"], We=HANDLE["We"], r_safe=[m.cfg.r_safe] * no, r_hit=[HANDLE["r_hit"]] * no)
        for n, a in src.items():
            setattr(self, n, alloc.f64(*a.shape)); put(getattr(self, n), a)
            setattr(self, "slot_" + n, alloc.f64(rows, a.shape[1])); put(getattr(self, "slot_" + n), np.tile(np.asarray(preset[n], dtype=np.float64), (rows, 1)))
        self.mask = alloc.i32(count); put(self.mask, sv.pack_obstacle_mask(f["active"]).view(np.int32))
        self.slot_mask = alloc.i32(rows, init=(1 << no) - 1)
        self.bounds = alloc.f64(count, 12); put(self.bounds, sv.pack_instance_bounds(m.cfg, count, **f["bounds"]))
        self.slot_bounds = alloc.f64(rows, 12); put(self.slot_bounds, sv.pack_instance_bounds(m.cfg, rows))
        self.log = alloc.i32(rows, 4); put(self.log, np.tile(np.array([0, 0, -1, 0], dtype=np.int32), (rows, 1)))
        self.res_log = alloc.i32(count, 3, init=-1)
        m.set_instance_params(W=self.slot_W, We=self.slot_We, r_safe=self.slot_r_safe, r_hit=self.slot_r_hit)
        m.set_obstacle_mask(self.slot_mask)
        m.set_instance_bounds_dev(self.slot_bounds)
        m.set_refill_tables_dev(W=self.W, We=self.We, r_safe=self.r_safe, r_hit=self.r_hit, mask=self.mask, bounds=self.bounds, slot_W=self.slot_W,
                                slot_We=self.slot_We, slot_r_safe=self.slot_r_safe, slot_r_hit=self.slot_r_hit, slot_mask=self.slot_mask,
                                slot_bounds=self.slot_bounds, log=self.log, res_log=self.res_log)
        self.names = TABLE_ARRAYS
        if capacity is not None:
            from mpc_gpu import _lib
            self.ring_state = alloc.i32(capacity, _lib.lib().mpc_noise_state_words()); self.ring_obst = alloc.f64(capacity, no, 4)
            self.ring_tag = alloc.i32(capacity, init=-1); self.seed_src = alloc.i32(count, init=-1)
            m.episode_ring_dev(capacity, self.ring_state, self.ring_obst, self.ring_tag, self.seed_src)
            self.names = TABLE_ARRAYS + RING_ARRAYS

    def snapshot(self, rows=slice(None)):
        """host copies of the per-slot tables and the log (rows `rows`) and of the ring arrays (whole); the caller synchronises"""
        return {n: (getattr(self, n)[rows] if n in TABLE_ARRAYS else getattr(self, n)).cpu().numpy().copy() for n in self.names}
