"""Test infrastructure of the SQP loop (mpc_set_sqp; test_sqp_host.py, test_gpu_sqp.py): per kernel family the smallest shapes that reach a level-5
instantiation, one batch of twelve instances from the cold guess, and the reference -- the oracle's K-fold sequence of single RTI solves stopped by the
rule of include/mpc_gpu.h.  Imports without torch or a GPU; the oracle is passed in.  No test functions here.

The stop rule (one instance): for k = 1, 2, ... solve once from the current iterate; end behind iteration k when its status is 4 (the iterate stays that
of iteration k - 1), or k == K, or the applied step has max-norm <= step_tol (every entry of dX and dU)."""
import hashlib

import numpy as np

from feature_kernel_cases import HORIZON
from helpers import oracle_P, random_batch

B = 12
K = 6                # SQP iterations per launch at most
NAN_INSTANCE = 5     # its x0 holds a NaN: status 4 at once, one iteration, the iterate untouched
IDLE_INSTANCE = 1    # the fused form: its episode is over, it runs nothing

POOL = 300           # a case's instances are picked out of random_batch(POOL, n_obst, seed)

# family, lanes per stage (one lane per stage: 1), row capacity = obstacles, the seed of the pool, the instances picked from it and the step tolerance.
# The full Gauss-Newton step contracts slowly (about x 0.8 .. 0.9 per iteration), so in a random batch nearly every instance either stops at once or
# runs all K iterations and has a norm near any tolerance on its way.  The picks are the pool's instances whose step norm drops by more than a factor
# five in one iteration -- at different iterations -- beside instances that stop at once and instances that run all K; step_tol lies in the gap.
# Found by running the oracle over the pool; test_sqp_host.py holds the conditions (no norm of an iteration run within a factor two of step_tol,
# three or more different stop counts).  Position NAN_INSTANCE of `pick` is the instance whose x0 is given a NaN
CASES = [
    dict(id="split3-3", family="split", lps=3, cap=3, seed=11, step_tol=2.875, pick=[20, 22, 35, 95, 248, 299, 4, 8, 12, 13, 21, 24]),
    dict(id="split3-10", family="split", lps=3, cap=10, seed=12, step_tol=2.081, pick=[26, 39, 12, 3, 289, 297, 6, 7, 8, 9, 13, 15]),
    dict(id="split2-3", family="split", lps=2, cap=3, seed=13, step_tol=2.683, pick=[1, 5, 254, 10, 201, 290, 22, 25, 29, 42, 52, 58]),
    dict(id="split2-10", family="split", lps=2, cap=10, seed=14, step_tol=1.252, pick=[21, 103, 231, 60, 239, 298, 1, 2, 4, 5, 7, 10]),
    dict(id="one-3", family="one", lps=1, cap=3, seed=15, step_tol=2.282, pick=[10, 15, 153, 198, 0, 282, 5, 9, 29, 39, 33, 34]),
    dict(id="one-10", family="one", lps=1, cap=10, seed=16, step_tol=2.562, pick=[4, 15, 14, 102, 291, 299, 246, 0, 3, 5, 7, 9]),
    dict(id="wide-20", family="wide", lps=2, cap=20, seed=17, step_tol=1.374, pick=[46, 200, 99, 165, 0, 299, 1, 5, 8, 11, 12, 13]),
    dict(id="wide-32", family="wide", lps=2, cap=32, seed=18, step_tol=2.683, pick=[166, 59, 107, 244, 0, 299, 1, 2, 3, 4, 5, 8]),
    # the five-obstacle rows, so that the loop's back edge runs in every one of the eleven level-5 instantiations
    dict(id="split3-5", family="split", lps=3, cap=5, seed=19, step_tol=3.081, pick=[10, 22, 18, 26, 188, 296, 112, 2, 3, 6, 8, 11]),
    dict(id="split2-5", family="split", lps=2, cap=5, seed=20, step_tol=1.771, pick=[18, 35, 252, 86, 192, 296, 0, 10, 16, 17, 20, 25]),
    dict(id="one-5", family="one", lps=1, cap=5, seed=21, step_tol=1.652, pick=[18, 39, 243, 281, 249, 298, 7, 11, 14, 20, 24, 25]),
]
# GPU self-consistency only (test_gpu_sqp.py, no oracle tolerance): with the interior point capped at 12 iterations these instances of a 200-instance
# pool end an early SQP iteration with status 2 (the step is applied, the loop goes on) and a later one with status 0 -- found by running the oracle
# over the pool (31 of its 200 instances do).  step_tol = 0: every instance runs all K iterations
STATUS2 = dict(id="status2", family="split", lps=3, cap=3, seed=31, pool=200, step_tol=0.0, cfg=dict(qp_iter_max=12),
               pick=[5, 17, 31, 34, 41, 0, 47, 23, 74, 95, 107, 1])
for _c in CASES + [STATUS2]:
    assert len(_c["pick"]) == B
    _c["N"] = HORIZON[("wide", _c["cap"])] if _c["family"] == "wide" else HORIZON[(_c["family"], _c["lps"])]
    _c["no"] = _c["cap"]
    _c["name"] = {"split": f"rti_split_kernel<{_c['cap']}, {_c['lps']}, false, true, false",
                  "one": f"rti_solve_kernel<{_c['cap']}, 64, 3, true",
                  "wide": f"rti_wide_kernel<{_c['cap']}, 2, true"}[_c["family"]] + ", true" * 5 + ">"
IDS = [c["id"] for c in CASES]


def case(cid):
    return next(c for c in CASES + [STATUS2] if c["id"] == cid)


_INPUTS, _REFERENCE = {}, {}


def inputs(orc, c):
    """x0, goal, obst, the explicit look-ahead P and the cold guess (X0, U0) of the case's batch; computed once per case and not to be written to"""
    if c["id"] not in _INPUTS:
        N, no = c["N"], c["no"]
        cfg = orc.config(N, no, 0.1 * N, **c.get("cfg", {}))
        x0, goal, obst = (np.ascontiguousarray(a[c["pick"]]) for a in random_batch(c.get("pool", POOL), no, seed=c["seed"]))
        x0[:, 3:] = 0.0
        P = oracle_P(orc, cfg, obst)
        X0, U0 = zip(*[orc.initial_guess(cfg, x) for x in x0])
        X0, U0 = np.stack(X0), np.stack(U0)
        x0[NAN_INSTANCE, 1] = np.nan          # (behind the guess: the iterate itself is finite, the solve must still refuse)
        _INPUTS[c["id"]] = dict(N=N, no=no, cfg=cfg, x0=x0, goal=goal, obst=obst, P=P, X0=X0, U0=U0)
    return _INPUTS[c["id"]]


NAN_FILLER_AFTER = 3      # the filler with a NaN in x0 is the third filler behind the pick's NaN instance


def embedded(orc, c, Bs, pos):
    """The case's batch inside one of Bs instances that the instance scheduler deals (feature_kernel_cases.embed): the twelve picks at rows pos with
    the handle's own feature values -- the goal as their reference at offset 0, the config's weights, radii and bounds, every obstacle present --
    so that oracle_sequence stays their reference; the fillers with feature rows of their own (a level-5 kernel reads every per-instance table), one
    of them with a NaN in x0.  X0, U0: the cold guess of every row.  Computed once per (case, Bs) and not to be written to"""
    from feature_kernel_cases import B as FB, embed
    from instance_bounds_cases import DEFAULTS, per_instance
    key = ("embedded", c["id"], Bs)
    if key not in _INPUTS:
        assert FB == B
        inp = inputs(orc, c)
        N, no, cfg = inp["N"], inp["no"], inp["cfg"]
        T = N + 6
        yref = np.zeros((B, T, 6)); yref[:, :, :2] = inp["goal"][:, None, :]
        own = dict(N=N, no=no, level=4, T=T, x0=inp["x0"], goal=inp["goal"], obst=inp["obst"], P=inp["P"], noise=np.zeros((B, no, 2)),
                   ep_flags=np.zeros(B, np.int32), yref=yref, offset=np.zeros(B, np.int32),
                   W=np.tile([cfg.W[k] for k in range(6)], (B, 1)), We=np.tile([cfg.We[k] for k in range(4)], (B, 1)),
                   r_safe=np.full((B, no), float(cfg.r_safe)), mask=np.ones((B, no), bool), bounds=per_instance([DEFAULTS], np.zeros(B, int)))
        e = embed(orc, own, Bs, pos, with_P=True)
        e["ep_flags"] = np.zeros(Bs, np.int32)      # (a plain solve: nothing idles)
        X0, U0 = zip(*[orc.initial_guess(cfg, x) for x in e["x0"]])
        e["X0"], e["U0"] = np.stack(X0), np.stack(U0)
        e["X0"][pos], e["U0"][pos] = inp["X0"], inp["U0"]
        e["nan_filler"] = int(np.nonzero(e["filler"] & (np.arange(Bs) > pos[NAN_INSTANCE]))[0][NAN_FILLER_AFTER - 1])
        e["x0"][e["nan_filler"], 1] = np.nan         # (behind the guess, as the pick's)
        _INPUTS[key] = e
    return _INPUTS[key]


def step_norm(Xa, Ua, Xb, Ub):
    """max-norm of the step between two iterates of one instance"""
    return float(max(np.abs(Xb - Xa).max(), np.abs(Ub - Ua).max()))


def _digest(a):
    return None if a is None else hashlib.sha1(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def oracle_sequence(orc, c, step_tol=None, max_iter=K, alpha=None, P=None):
    """The reference: per instance the oracle's single solves stopped by the rule above.  alpha: an explicit slack schedule (B, N + 1), every solve
    of instance b run with alpha[b]; P: a look-ahead (B, N + 1, n_obst, 2) in place of the case's own (slack_schedule_cases).
    Returns dict(X, U, u0, cost, status, iters (the sum), sqp_iters,
    norms (B, max_iter) -- NaN where an iteration did not run or failed --, statuses (B, max_iter) -- -1 where it did not run --, iterates: per
    instance the list of (X, U) in front of every iteration run).  Computed once per (case, step_tol, max_iter) and not to be written to"""
    step_tol = c["step_tol"] if step_tol is None else step_tol
    key = (c["id"], float(step_tol), int(max_iter), _digest(alpha), _digest(P))
    if key in _REFERENCE:
        return _REFERENCE[key]
    inp = inputs(orc, c)
    cfg, N = inp["cfg"], inp["N"]
    P = inp["P"] if P is None else P
    out = dict(X=inp["X0"].copy(), U=inp["U0"].copy(), u0=np.zeros((B, 2)), cost=np.zeros(B), status=np.zeros(B, np.int32), iters=np.zeros(B, np.int32),
               sqp_iters=np.zeros(B, np.int32), norms=np.full((B, max_iter), np.nan), statuses=np.full((B, max_iter), -1, np.int32), iterates=[[] for _ in range(B)])
    for b in range(B):
        X, U = inp["X0"][b].copy(), inp["U0"][b].copy()
        for k in range(1, max_iter + 1):
            out["iterates"][b].append((X.copy(), U.copy()))
            r = orc.rti_solve(cfg, inp["x0"][b], P[b], inp["goal"][b], X, U, alpha=None if alpha is None else alpha[b])
            out["statuses"][b, k - 1] = r["status"]; out["iters"][b] += r["iters"]; out["sqp_iters"][b] = k
            out["status"][b], out["u0"][b], out["cost"][b] = r["status"], r["u0"], r["cost"]
            if r["status"] == 4:
                break
            nrm = step_norm(X, U, r["X"], r["U"])
            out["norms"][b, k - 1] = nrm
            X, U = r["X"], r["U"]
            if nrm <= step_tol:
                break
        out["X"][b], out["U"][b] = X, U
    _REFERENCE[key] = out
    return out


def finite_instances():
    return np.array([b for b in range(B) if b != NAN_INSTANCE])
