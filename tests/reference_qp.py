"""Numpy side of the per-stage reference (mpc_set_reference): the row each stage tracks, the QP gradient shifted from the goal's reference to it,
and the LS cost against it.  Test infrastructure, independent of the kernels."""
import numpy as np


def stage_rows(yref, offset, N):
    """(N+1, 6) reference rows of one instance: row min(offset + i, T - 1) for stage i, the terminal row's input columns zero"""
    T = yref.shape[0]
    R = np.array([yref[min(int(offset) + i, T - 1)] for i in range(N + 1)], dtype=np.float64)
    R[N, 4:] = 0.0
    return R


def goal_rows(goal, N):
    """the reference the solver derives from the goal: [g_x, g_y, 0, 0, 0, 0] at every stage (robot_ocp_problem.py:59-83)"""
    R = np.zeros((N + 1, 6))
    R[:, :2] = goal
    return R


def _weights(cfg):
    dt = cfg.Tf / cfg.N
    cs = dt if cfg.cost_scale_dt else 1.0
    return np.array([cs * cfg.W[k] for k in range(6)]), np.array([cfg.We[k] for k in range(4)])


def shift_gradient(cfg, q, goal, R):
    """export_qp's q (built against the goal) moved to the per-stage reference R (N+1, 6): g += cs W (yref_goal - yref_i), variable order
    (du_i, dx_{i+1}) per block as in orc_export_qp; z order of a state block (x, y, psi, v, om)"""
    N = cfg.N
    Wg, Weg = _weights(cfg)
    G = goal_rows(goal, N)
    g = q["g"].copy()
    for i in range(N):
        d = G[i] - R[i]
        g[7 * i + 0] += Wg[4] * d[4]
        g[7 * i + 1] += Wg[5] * d[5]
        st = i + 1
        W = Wg if st < N else Weg
        d = G[st] - R[st]
        g[7 * i + 2] += W[0] * d[0]
        g[7 * i + 3] += W[1] * d[1]
        g[7 * i + 5] += W[2] * d[2]
        g[7 * i + 6] += W[3] * d[3]
    out = dict(q)
    out["g"] = g
    return out


def stage_gradient(cfg, X, U, R):
    """the LS part of the linearisation's gradient q[N+1][7] (order ua, ual, x, y, psi, v, om) against R, as mpc_linearize_dev writes it"""
    N = cfg.N
    Wg, Weg = _weights(cfg)
    q = np.zeros((N + 1, 7))
    for i in range(N + 1):
        x = X[i]
        if i < N:
            q[i, 0] = Wg[4] * (U[i, 0] - R[i, 4]); q[i, 1] = Wg[5] * (U[i, 1] - R[i, 5])
            W = Wg
        else:
            W = Weg
        q[i, 2] = W[0] * (x[0] - R[i, 0]); q[i, 3] = W[1] * (x[1] - R[i, 1])
        q[i, 5] = W[2] * (x[3] - R[i, 2]); q[i, 6] = W[3] * (x[4] - R[i, 3])
    return q


def ls_cost(cfg, X, U, R):
    """0.5 sum_i |y_i - yref_i|^2_W (stages < N weighted by cs W, the terminal by W_e)"""
    N = cfg.N
    Wg, Weg = _weights(cfg)
    J = 0.0
    for i in range(N + 1):
        e = np.array([X[i, 0] - R[i, 0], X[i, 1] - R[i, 1], X[i, 3] - R[i, 2], X[i, 4] - R[i, 3]])
        if i < N:
            eu = U[i] - R[i, 4:]
            J += 0.5 * (np.sum(Wg[:4] * e * e) + np.sum(Wg[4:] * eu * eu))
        else:
            J += 0.5 * np.sum(Weg * e * e)
    return J


def slack_penalty(cfg, x0, goal, X, P):
    """exact penalty of the obstacle violation at the iterate, with the built-in slack schedule (robot_ocp_problem.py:145-152)"""
    N, no = cfg.N, cfg.n_obst
    dt = cfg.Tf / N
    d = np.array([x0[0] - goal[0], x0[1] - goal[1], x0[3], x0[4]])
    a = cfg.slack_a * (np.sum(d * d) + cfg.slack_b)
    J = 0.0
    for i in range(N + 1):
        z = a * (N - i) / N * (dt if (cfg.slack_scale_dt and i < N) else 1.0)
        for j in range(no):
            h = (X[i, 0] - P[i, j, 0]) ** 2 + (X[i, 1] - P[i, j, 1]) ** 2 - cfg.r_safe ** 2
            v = -h if h < 0 else 0.0
            J += z * (v + 0.5 * v * v)
    return J
