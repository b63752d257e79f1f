"""Numpy side of the per-instance parameters (mpc_set_instance_params): an exported QP rewritten to other cost weights and per-obstacle radii, the
linearisation's q and hval with them, and the reported cost.  Test infrastructure, independent of the kernels."""
import numpy as np


def scalings(cfg):
    """(cs, LM term of the stages, LM term of the terminal stage), as make_params forms them"""
    dt = cfg.Tf / cfg.N
    return (dt if cfg.cost_scale_dt else 1.0), (cfg.lm * dt if cfg.lm_scaled else cfg.lm), cfg.lm


def derived(cfg, W, We):
    """(Hd_stage[7], Hd_term[5], Wg[6], Weg[4]) of one instance: z order (ua, ual, x, y, psi, v, om) of the diagonals, y order (x, y, v, om, ua, ual) of
    the weights"""
    cs, lms, lmt = scalings(cfg)
    W, We = np.asarray(W, float), np.asarray(We, float)
    hs = np.array([cs * W[4] + lms, cs * W[5] + lms, cs * W[0] + lms, cs * W[1] + lms, lms, cs * W[2] + lms, cs * W[3] + lms])
    ht = np.array([We[0] + lmt, We[1] + lmt, lmt, We[2] + lmt, We[3] + lmt])
    return hs, ht, cs * W, We.copy()


def retarget_qp(cfg, qp, W, We, r):
    """orc.export_qp(cfg, ...) rewritten to the weights W (6,), We (4,) and the radii r (n_obst,) or a scalar.  Variable order (du_i, dx_{i+1}) per block,
    a state block in z order (x, y, psi, v, om).  The Hessian is diagonal: its entries become cs W + lm; the gradient is W (y - yref) entry by entry, so
    it is rescaled by new over old weight (the oracle's weights must be non-zero where the new ones are); obstacle rows are ordered [stage 1..][obstacle]
    (every stage that has a slack weight) with value |p - o_j|^2 - r_safe^2, so a radius moves hs by cfg.r_safe^2 - r_j^2 and leaves the rows' gradients alone."""
    N, no = cfg.N, cfg.n_obst
    hs, ht, wg, we = derived(cfg, W, We)
    _, _, wg0, we0 = derived(cfg, [cfg.W[k] for k in range(6)], [cfg.We[k] for k in range(4)])
    H, g = qp["H"].copy(), qp["g"].copy()

    def scale(v, new, old):
        if new != old:
            if old == 0.0:
                raise ValueError("cannot rescale a gradient entry whose weight in the exported QP is zero")
            g[v] *= new / old

    for i in range(N):
        b = 7 * i
        H[b, b], H[b + 1, b + 1] = hs[0], hs[1]
        scale(b, wg[4], wg0[4]); scale(b + 1, wg[5], wg0[5])
        term = (i + 1 == N)
        d = ht if term else hs[2:]
        for k in range(5):
            H[b + 2 + k, b + 2 + k] = d[k]
        w, w0 = (we, we0) if term else (wg, wg0)
        scale(b + 2, w[0], w0[0]); scale(b + 3, w[1], w0[1]); scale(b + 5, w[2], w0[2]); scale(b + 6, w[3], w0[3])
    out = dict(qp)
    out["H"], out["g"] = H, g
    rr = np.broadcast_to(np.asarray(r, float), (no,))
    hsr = qp["hs"].copy()
    stages = len(hsr) // no      # (stages 1 .. N - 1 with the built-in schedule: the terminal stage's slack weight is zero and its rows are not exported)
    if stages * no != len(hsr) or stages > N:
        raise ValueError(f"expected obstacle rows [stage 1..][obstacle] of at most {N} stages with {no} obstacles, got {len(hsr)}")
    hsr += np.tile(cfg.r_safe ** 2 - rr ** 2, stages)
    out["hs"] = hsr
    return out


def stage_gradient(cfg, X, U, goal, W, We):
    """q[N+1][7] of mpc_linearize_dev (order ua, ual, x, y, psi, v, om) against the goal with the instance's weights"""
    N = cfg.N
    _, _, wg, we = derived(cfg, W, We)
    q = np.zeros((N + 1, 7))
    for i in range(N + 1):
        w = wg if i < N else we
        if i < N:
            q[i, 0] = wg[4] * U[i, 0]; q[i, 1] = wg[5] * U[i, 1]
        q[i, 2] = w[0] * (X[i, 0] - goal[0]); q[i, 3] = w[1] * (X[i, 1] - goal[1])
        q[i, 5] = w[2] * X[i, 3]; q[i, 6] = w[3] * X[i, 4]
    return q


def hval(X, P, r):
    """hval[N+1][n_obst] of mpc_linearize_dev with the radii r (n_obst,)"""
    d = X[:, None, :2] - P
    return (d ** 2).sum(axis=2) - np.asarray(r, float)[None, :] ** 2


def cost(cfg, x0, goal, X, U, P, W, We, r):
    """the reported cost: LS cost with the instance's weights plus the exact penalty of the violation of its obstacles' radii (built-in slack schedule)"""
    N, no = cfg.N, cfg.n_obst
    _, _, wg, we = derived(cfg, W, We)
    dt = cfg.Tf / N
    J = 0.0
    for i in range(N + 1):
        e = np.array([X[i, 0] - goal[0], X[i, 1] - goal[1], X[i, 3], X[i, 4]])
        J += 0.5 * (np.sum(wg[:4] * e * e) + np.sum(wg[4:] * U[i] * U[i])) if i < N else 0.5 * np.sum(we * e * e)
    d = np.array([x0[0] - goal[0], x0[1] - goal[1], x0[3], x0[4]])
    a = cfg.slack_a * (np.sum(d * d) + cfg.slack_b)
    h = hval(X, P, np.broadcast_to(np.asarray(r, float), (no,)))
    for i in range(N + 1):
        z = a * (N - i) / N * (dt if (cfg.slack_scale_dt and i < N) else 1.0)
        v = np.where(h[i] < 0, -h[i], 0.0)
        J += z * np.sum(v + 0.5 * v * v)
    return J


def draw_sets(rng, cfg, K, r_lo=1.6, r_hi=3.0):
    """K parameter sets: weights within 0.25x .. 4x of the config's (log-uniform), one radius per set in [r_lo, r_hi]"""
    W0 = np.array([cfg.W[k] for k in range(6)]); We0 = np.array([cfg.We[k] for k in range(4)])
    W = W0 * np.exp(rng.uniform(np.log(0.25), np.log(4.0), (K, 6)))
    We = We0 * np.exp(rng.uniform(np.log(0.25), np.log(4.0), (K, 4)))
    return W, We, rng.uniform(r_lo, r_hi, K)
