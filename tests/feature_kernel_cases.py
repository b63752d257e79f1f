"""Test infrastructure of the feature-level kernel sweep (test_feature_kernel_cases_host.py, test_gpu_every_feature_kernel.py): the 78 solve
instantiations of csrc/solve_dispatch.hpp at feature levels 1 to 4 (REF, IPAR, OSEL, IBND), a handle that reaches each, and per case one batch of
twelve instances in four groups of three whose feature values differ group by group, so that the oracle -- which knows one config -- can be asked
about each group; `embed` puts those twelve into a batch that the instance scheduler deals (test_gpu_feature_scheduling.py).  Imports without torch or a
GPU; the oracle is passed in.

The matrix: levels 1 and 2 have, each, one lane per stage <3|5|10, 64, 3, false|true> (6), the stage split
<3|5|10, 2|3> x {plain, two wavefronts per SIMD, run-time row count} (18) and the multi-wavefront kernel <20|32, 2, false|true> (4); levels 3 and 4
have the run-time row count alone (3 + 6 + 2)."""
import numpy as np

from helpers import oracle_P, random_batch
from instance_bounds_cases import as_cfg, draw_bounds, per_instance
from off_default_cases import IP

B = 12
GROUPS = 4
FAMILIES = ("one", "split", "wide")
LEVELS = (1, 2, 3, 4)
LEVEL_SUFFIX = {1: ", true", 2: ", true, true", 3: ", true, true, true", 4: ", true, true, true, true"}

# obstacle counts that fill a row capacity / that leave it partly empty (the run-time row count)
FULL = {3: 3, 5: 5, 10: 10, 20: 20, 32: 32}
PARTIAL = {3: 2, 5: 4, 10: 7, 20: 15, 32: 27}
DECOY_RADIUS = 1.5      # added to the radius entry of an absent obstacle, which no kernel may read for a present one
HORIZON = {("split", 3): 20, ("split", 2): 30, ("one", 1): 50, ("wide", 20): 20, ("wide", 32): 31}

# the 78 names, written out (test_feature_kernel_cases_host.py compares the enumeration with this list)
NAMES = [
    "rti_solve_kernel<3, 64, 3, false, true>", "rti_solve_kernel<3, 64, 3, true, true>",
    "rti_solve_kernel<5, 64, 3, false, true>", "rti_solve_kernel<5, 64, 3, true, true>",
    "rti_solve_kernel<10, 64, 3, false, true>", "rti_solve_kernel<10, 64, 3, true, true>",
    "rti_split_kernel<3, 2, false, false, false, true>", "rti_split_kernel<3, 2, true, false, false, true>", "rti_split_kernel<3, 2, false, true, false, true>",
    "rti_split_kernel<3, 3, false, false, false, true>", "rti_split_kernel<3, 3, true, false, false, true>", "rti_split_kernel<3, 3, false, true, false, true>",
    "rti_split_kernel<5, 2, false, false, false, true>", "rti_split_kernel<5, 2, true, false, false, true>", "rti_split_kernel<5, 2, false, true, false, true>",
    "rti_split_kernel<5, 3, false, false, false, true>", "rti_split_kernel<5, 3, true, false, false, true>", "rti_split_kernel<5, 3, false, true, false, true>",
    "rti_split_kernel<10, 2, false, false, false, true>", "rti_split_kernel<10, 2, true, false, false, true>", "rti_split_kernel<10, 2, false, true, false, true>",
    "rti_split_kernel<10, 3, false, false, false, true>", "rti_split_kernel<10, 3, true, false, false, true>", "rti_split_kernel<10, 3, false, true, false, true>",
    "rti_wide_kernel<20, 2, false, true>", "rti_wide_kernel<20, 2, true, true>",
    "rti_wide_kernel<32, 2, false, true>", "rti_wide_kernel<32, 2, true, true>",
    "rti_solve_kernel<3, 64, 3, false, true, true>", "rti_solve_kernel<3, 64, 3, true, true, true>",
    "rti_solve_kernel<5, 64, 3, false, true, true>", "rti_solve_kernel<5, 64, 3, true, true, true>",
    "rti_solve_kernel<10, 64, 3, false, true, true>", "rti_solve_kernel<10, 64, 3, true, true, true>",
    "rti_split_kernel<3, 2, false, false, false, true, true>", "rti_split_kernel<3, 2, true, false, false, true, true>", "rti_split_kernel<3, 2, false, true, false, true, true>",
    "rti_split_kernel<3, 3, false, false, false, true, true>", "rti_split_kernel<3, 3, true, false, false, true, true>", "rti_split_kernel<3, 3, false, true, false, true, true>",
    "rti_split_kernel<5, 2, false, false, false, true, true>", "rti_split_kernel<5, 2, true, false, false, true, true>", "rti_split_kernel<5, 2, false, true, false, true, true>",
    "rti_split_kernel<5, 3, false, false, false, true, true>", "rti_split_kernel<5, 3, true, false, false, true, true>", "rti_split_kernel<5, 3, false, true, false, true, true>",
    "rti_split_kernel<10, 2, false, false, false, true, true>", "rti_split_kernel<10, 2, true, false, false, true, true>", "rti_split_kernel<10, 2, false, true, false, true, true>",
    "rti_split_kernel<10, 3, false, false, false, true, true>", "rti_split_kernel<10, 3, true, false, false, true, true>", "rti_split_kernel<10, 3, false, true, false, true, true>",
    "rti_wide_kernel<20, 2, false, true, true>", "rti_wide_kernel<20, 2, true, true, true>",
    "rti_wide_kernel<32, 2, false, true, true>", "rti_wide_kernel<32, 2, true, true, true>",
    "rti_solve_kernel<3, 64, 3, true, true, true, true>", "rti_solve_kernel<5, 64, 3, true, true, true, true>", "rti_solve_kernel<10, 64, 3, true, true, true, true>",
    "rti_split_kernel<3, 2, false, true, false, true, true, true>", "rti_split_kernel<3, 3, false, true, false, true, true, true>",
    "rti_split_kernel<5, 2, false, true, false, true, true, true>", "rti_split_kernel<5, 3, false, true, false, true, true, true>",
    "rti_split_kernel<10, 2, false, true, false, true, true, true>", "rti_split_kernel<10, 3, false, true, false, true, true, true>",
    "rti_wide_kernel<20, 2, true, true, true, true>", "rti_wide_kernel<32, 2, true, true, true, true>",
    "rti_solve_kernel<3, 64, 3, true, true, true, true, true>", "rti_solve_kernel<5, 64, 3, true, true, true, true, true>", "rti_solve_kernel<10, 64, 3, true, true, true, true, true>",
    "rti_split_kernel<3, 2, false, true, false, true, true, true, true>", "rti_split_kernel<3, 3, false, true, false, true, true, true, true>",
    "rti_split_kernel<5, 2, false, true, false, true, true, true, true>", "rti_split_kernel<5, 3, false, true, false, true, true, true, true>",
    "rti_split_kernel<10, 2, false, true, false, true, true, true, true>", "rti_split_kernel<10, 3, false, true, false, true, true, true, true>",
    "rti_wide_kernel<20, 2, true, true, true, true, true>", "rti_wide_kernel<32, 2, true, true, true, true, true>",
]


def _tf(v):
    return "true" if v else "false"


def enumerate_cases():
    """[dict(family, level, N, no, overrides, name)] for the 78 rows, from the matrix's rule.  overrides: dict(waves=2) for two wavefronts per SIMD,
    else {}.  Below level 3 a handle runs the run-time row count when its obstacles leave the capacity partly empty; at levels 3 and 4 every handle
    does (the mask is a run-time row count by nature), and the sweep takes the partly empty handle at level 3 and the full one at level 4."""
    out = []
    for level in LEVELS:
        kinds = ((False, {}), (True, {})) if level <= 2 else ((True, {}),)
        for cap in (3, 5, 10):
            for masked, ov in kinds:
                out.append(dict(family="one", level=level, N=HORIZON["one", 1], cap=cap, masked=masked, overrides=ov,
                                name=f"rti_solve_kernel<{cap}, 64, 3, {_tf(masked)}{LEVEL_SUFFIX[level]}>"))
        for cap in (3, 5, 10):
            for lps in (2, 3):
                split_kinds = ((False, {}), (False, dict(waves=2)), (True, {})) if level <= 2 else ((True, {}),)
                for masked, ov in split_kinds:
                    out.append(dict(family="split", level=level, N=HORIZON["split", lps], cap=cap, masked=masked, overrides=ov,
                                    name=f"rti_split_kernel<{cap}, {lps}, {_tf(bool(ov))}, {_tf(masked)}, false{LEVEL_SUFFIX[level]}>"))
        for cap in (20, 32):
            for masked, ov in kinds:
                out.append(dict(family="wide", level=level, N=HORIZON["wide", cap], cap=cap, masked=masked, overrides=ov,
                                name=f"rti_wide_kernel<{cap}, 2, {_tf(masked)}{LEVEL_SUFFIX[level]}>"))
    for c in out:
        partial = c["masked"] if c["level"] <= 2 else c["level"] == 3
        c["no"] = (PARTIAL if partial else FULL)[c["cap"]]
    return out


def cases_of(family, level):
    return [c for c in enumerate_cases() if c["family"] == family and c["level"] == level]


def configure(s, case):
    """the case's lane mapping on a fresh handle (the features decide the rest)"""
    if case["overrides"].get("waves"):
        s.set_waves_per_simd(case["overrides"]["waves"])


# ---------------------------------------------------------------------------------------------------------------- inputs
def inputs(orc, case):
    """Everything one case runs on.  The world (x0, goal, obst, noise, the groups) depends on (N, n_obst) alone; the feature values on (N, n_obst) and
    the feature, so a level adds its feature to what the level below ran with.  Arrays per instance (what the handle is given) and values per group
    (what the oracle's config is given): group 0 holds the handle's own values, a full mask and the default bounds."""
    N, no, level = case["N"], case["no"], case["level"]
    T = N + 6
    x0, goal, obst = random_batch(B, no, seed=100 * N + no)
    x0[:, 3:] = 0.0
    x0[0, :2] = goal[0] + 0.05                       # instance 0 reaches its goal in this step: flag 1, step counter not advanced
    noise = np.random.default_rng(N * 31 + no).standard_normal((B, no, 2))
    ep_flags = np.zeros(B, np.int32); ep_flags[1] = 1      # instance 1 has finished its episode: it idles
    menu, group = draw_bounds(np.random.default_rng([N, no, 4]), B, GROUPS)
    base = orc.config(N, no, 0.1 * N)
    W0, We0, r0 = np.array([base.W[k] for k in range(6)]), np.array([base.We[k] for k in range(4)]), float(base.r_safe)
    g = [dict(W=W0.copy(), We=We0.copy(), r_safe=np.full(no, r0), mask=np.ones(no, bool), bounds=menu[0]) for _ in range(GROUPS)]
    # level >= 1: the goal problem behind a per-instance offset, a decoy (the goal moved by (+5, -5)) in front of it
    rng = np.random.default_rng([N, no, 1])
    offset = np.zeros(B, np.int32)
    own = np.nonzero(group != 0)[0]
    while len(set(offset[own].tolist())) < 2:
        offset[own] = rng.integers(0, 4, len(own))
    yref = np.zeros((B, T, 6))
    yref[:, :, :2] = goal[:, None, :]
    for b in range(B):
        yref[b, :offset[b], :2] += (5.0, -5.0)
    if level >= 2:
        rng = np.random.default_rng([N, no, 2])
        for k in range(1, GROUPS):
            g[k]["W"] = np.array(IP["W"]) * rng.uniform(0.5, 3.0, 6)
            g[k]["We"] = np.array(IP["We"]) * rng.uniform(0.5, 3.0, 4)
            g[k]["r_safe"] = rng.uniform(1.6, 3.0, no)       # a radius per obstacle: the oracle is given them (oracle.obstacle_radii)
    # level >= 3: a mask per group -- at least one obstacle kept, not all kept in two groups or more, obstacle 0 absent in one or more (its radius entry,
    # a decoy, is then the first of the instance's row)
    if level >= 3:
        rng = np.random.default_rng([N, no, 3])
        while True:
            masks = [rng.uniform(size=no) < 0.6 for _ in range(1, GROUPS)]
            if all(m.any() for m in masks) and sum(not m.all() for m in masks) >= 2 and any(not m[0] for m in masks):
                break
        for k in range(1, GROUPS):
            g[k]["mask"] = masks[k - 1]
    if level >= 4:
        for k in range(1, GROUPS):
            g[k]["bounds"] = menu[k]
    return dict(N=N, no=no, level=level, T=T, x0=x0, goal=goal, obst=obst, noise=noise, ep_flags=ep_flags, group=group, groups=g, thr0=float(base.thr0),
                yref=yref, offset=offset,
                W=np.stack([g[k]["W"] for k in group]), We=np.stack([g[k]["We"] for k in group]),
                r_safe=np.stack([np.where(g[k]["mask"], g[k]["r_safe"], g[k]["r_safe"] + DECOY_RADIUS) for k in group]),
                mask=np.stack([g[k]["mask"] for k in group]),
                bounds=per_instance([e["bounds"] for e in g], group), P=oracle_P(orc, base, obst))


# ---------------------------------------------------------------------------------------------------------------- a scheduled batch around a case
EMBEDDED = ("x0", "goal", "obst", "noise", "ep_flags", "yref", "offset", "W", "We", "r_safe", "mask")      # per-instance arrays (and bounds, alpha, P, X0, U0)
FEATURE_ARRAYS = ("yref", "W", "We", "r_safe", "bounds", "alpha")      # every row its own: a neighbour's row is another problem


def positions(Bs):
    """where the twelve judged instances sit in a batch of Bs: case instance 0 at index 0, case instance 11 at Bs - 1, the others spread evenly"""
    pos = np.round(np.linspace(0, Bs - 1, B)).astype(np.int64)
    assert pos[0] == 0 and pos[-1] == Bs - 1 and len(set(pos.tolist())) == B
    return pos


def embed(orc, case_inputs, Bs, pos, alpha=None, with_P=False):
    """The case's twelve instances inside a batch of Bs that the instance scheduler deals: rows pos[0 .. 11] of every
    per-instance array are the case's own rows, bit for bit; the other Bs - 12 rows are fillers, random_batch(Bs, n_obst, seed) at rest, each with
    feature values of its own from the ranges of `inputs`' groups -- weights IP times U(0.5, 3), radii in U(1.6, 3.0) (a decoy added where the
    obstacle is absent), from level 3 on a mask that keeps one obstacle or more, a bound set of its own from draw_bounds' menu, an offset in 0 .. 3
    with the decoy in front of it, a row of slack_schedule_cases.schedule where `alpha` (the case's (12, N + 1) schedule) is given.  About one filler
    in a hundred starts idle.  with_P: the look-ahead of every row (the case's own at pos).  A slot index in place of the instance index
    therefore reads a valid row of a valid array that is another problem.  Returns the case's dict with the arrays replaced, `pos`, `case`
    (the inputs it came from) and `filler` (bool (Bs,))."""
    inp = case_inputs
    N, no, level, T = inp["N"], inp["no"], inp["level"], inp["T"]
    pos = np.asarray(pos, dtype=np.int64)
    assert pos.shape == (B,) and len(set(pos.tolist())) == B and pos.min() >= 0 and pos.max() < Bs
    rng = np.random.default_rng([N, no, level, Bs, 7])
    x0, goal, obst = random_batch(Bs, no, seed=[N, no, Bs, 6])
    x0[:, 3:] = 0.0
    filler = np.ones(Bs, bool); filler[pos] = False
    out = dict(x0=x0, goal=goal, obst=obst, noise=rng.standard_normal((Bs, no, 2)), ep_flags=np.zeros(Bs, np.int32))
    out["ep_flags"][rng.choice(np.nonzero(filler)[0], max(3, Bs // 100), replace=False)] = 1
    out["offset"] = rng.integers(0, 4, Bs).astype(np.int32)
    yref = np.zeros((Bs, T, 6))
    yref[:, :, :2] = goal[:, None, :]
    for b in range(Bs):
        yref[b, :out["offset"][b], :2] += (5.0, -5.0)
    out["yref"] = yref
    out["W"] = np.array(IP["W"]) * rng.uniform(0.5, 3.0, (Bs, 6))
    out["We"] = np.array(IP["We"]) * rng.uniform(0.5, 3.0, (Bs, 4))
    mask = np.ones((Bs, no), bool)
    if level >= 3:
        mask = rng.uniform(size=(Bs, no)) < 0.6
        mask[np.arange(Bs), rng.integers(0, no, Bs)] = True
    out["mask"] = mask
    r = rng.uniform(1.6, 3.0, (Bs, no))
    out["r_safe"] = np.where(mask, r, r + DECOY_RADIUS)
    menu, _ = draw_bounds(rng, Bs, Bs + 1)                # entry 0 is the handle's defaults, which the judged rows of group 0 hold
    bounds = per_instance(menu, np.arange(1, Bs + 1))
    if alpha is not None:
        from slack_schedule_cases import BUILTIN_ROW, schedule
        # the rows behind the schedule's special ones (the all-zero row, the terminal row, the built-in row: the case's own schedule has them)
        out["alpha"] = schedule(N, Bs + BUILTIN_ROW + 1, 1000 * level + 9, builtin=np.ones(N + 1))[BUILTIN_ROW + 1:]
        out["alpha"][pos] = alpha
    for k in EMBEDDED:
        out[k][pos] = inp[k]
    for k in bounds:
        bounds[k][pos] = inp["bounds"][k]
    out["bounds"] = bounds
    if with_P:
        out["P"] = oracle_P(orc, orc.config(N, no, 0.1 * N), obst)
        out["P"][pos] = inp["P"]
    return dict(inp, **out, pos=pos, filler=filler, case=inp, Bs=Bs)


def distinct_rows(emb, name):
    """(rows of array `name`, as a 2-D array) of an embedded batch: what test_feature_kernel_cases_host.py asks to be pairwise different"""
    a = emb[name]
    if name == "bounds":
        a = np.concatenate([a[k] for k in ("bx_lo", "bx_hi", "bu_lo", "bu_hi")], axis=1)
    return np.ascontiguousarray(a.reshape(a.shape[0], -1))


def group_problem(orc, inp, k):
    """(idx, cfg, P on the kept columns, radii of the kept obstacles or None) of group k: the oracle's config with the group's values.  From level 2 on
    the oracle's calls run inside `with orc.obstacle_radii(radii)`; the config's own radius is NaN then, so a call outside it cannot pass for one inside"""
    idx = np.nonzero(inp["group"] == k)[0]
    e = inp["groups"][k]
    kw = dict(thr0=inp["thr0"])
    if inp["level"] >= 2:
        kw.update(W=[float(v) for v in e["W"]], We=[float(v) for v in e["We"]], r_safe=float("nan"))
    if inp["level"] >= 4:
        kw.update(as_cfg(e["bounds"]))
    cfg = orc.config(inp["N"], int(e["mask"].sum()), 0.1 * inp["N"], **kw)
    radii = np.ascontiguousarray(e["r_safe"][e["mask"]]) if inp["level"] >= 2 else None
    return idx, cfg, np.ascontiguousarray(inp["P"][idx][:, :, e["mask"], :]), radii


def oracle_alone(orc, case, inp=None):
    """per group, the oracle on the case's inputs: a cold solve, then one from its own result.  Returns [(idx, cfg, first, second)]"""
    inp = inputs(orc, case) if inp is None else inp
    out = []
    for k in range(GROUPS):
        idx, cfg, Pk, radii = group_problem(orc, inp, k)
        X, U = zip(*[orc.initial_guess(cfg, x) for x in inp["x0"][idx]])
        with orc.obstacle_radii(radii):
            first = orc.rti_solve_batch(cfg, inp["x0"][idx], Pk, inp["goal"][idx], np.stack(X), np.stack(U))
            second = orc.rti_solve_batch(cfg, inp["x0"][idx], Pk, inp["goal"][idx], first["X"], first["U"])
        out.append((idx, cfg, first, second))
    return out


def bound_active(entry, N, X, U, tol=1e-6):
    """whether a solve (X (N + 1, 5), U (N, 2)) sits on one of the entry's bounds: the inputs of every stage, x, y, v, omega of stages 1 .. N - 1"""
    lo, hi = np.abs(U - entry["bu_lo"]) <= tol, np.abs(U - entry["bu_hi"]) <= tol
    s = X[1:N][:, [0, 1, 3, 4]]
    return bool(lo.any() or hi.any() or (np.abs(s - entry["bx_lo"]) <= tol).any() or (np.abs(s - entry["bx_hi"]) <= tol).any())
