"""Per-stage reference (mpc_set_reference) without a GPU: the header and the ctypes mirror, NULL-handle refusals, the shim's forwarding in its
default and stage_yref modes, and the numpy gradient shift against the oracle's exported QP."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from reference_qp import goal_rows, shift_gradient, stage_gradient, stage_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_reference_api():
    h = open(os.path.join(ROOT, "include", "mpc_gpu.h")).read()
    assert re.search(r"int mpc_set_reference\(mpc_handle \*h, int batch, int T, const double \*yref, const int32_t \*offset\);", h)
    assert re.search(r"int mpc_set_reference_dev\(mpc_handle \*h, int T, const double \*d_yref, int32_t \*d_offset\);", h)
    assert re.search(r"#define MPC_STEP_ADVANCE_REF 128\b", h)
    assert re.search(r"#define MPC_ABI_VERSION 7\b", h)


def test_mirror_binds_reference_api(built):
    import mpc_gpu
    L = mpc_gpu._lib
    assert L.STEP_ADVANCE_REF == 128
    assert L.SYMBOLS["mpc_set_reference"][1] == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    assert L.SYMBOLS["mpc_set_reference_dev"][1] == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib = L.lib()
    y = np.zeros((1, 3, 6))
    assert lib.mpc_set_reference(None, 1, 3, y.ctypes.data, None) == L.MPC_ERR_ARG
    assert b"null handle" in lib.mpc_last_error()
    assert lib.mpc_set_reference_dev(None, 3, None, None) == L.MPC_ERR_ARG


class FakeMpc:
    """records what the shim forwards"""
    def __init__(self, N):
        self.N, self.calls = N, []

    def set_reference(self, yref):
        self.calls.append(("set_reference", None if yref is None else np.array(yref)))

    def set_slack_schedule(self, a):
        self.calls.append(("set_slack_schedule", np.array(a)))

    def set_warmstart(self, X, U):
        self.calls.append(("set_warmstart", np.array(X), np.array(U)))

    def solve(self, x0, P, goal):
        self.calls.append(("solve", np.array(x0), np.array(P), np.array(goal)))
        return dict(status=np.zeros(1, np.int32), iters=np.ones(1, np.int32), cost=np.zeros(1), u0=np.zeros((1, 2)))

    def get_traj(self, B):
        return np.zeros((B, self.N + 1, 5)), np.zeros((B, self.N, 2))


def _shim(stage_yref, N=5):
    from mpc_gpu.acados_shim import AcadosOcpSolverShim
    f = FakeMpc(N)
    return AcadosOcpSolverShim(N, 2, 0.5, goal=(1.0, 2.0), mpc=f, stage_yref=stage_yref), f


def test_shim_default_mode_forwards_what_it_did():
    shim, f = _shim(False)
    shim.cost_set(3, "yref", [4.0, 5.0, 0.5, 0.1, 0.2, 0.3])     # position of any stage becomes the goal (defect D4 fix), the rest is dropped
    shim.solve()
    assert [c[0] for c in f.calls] == ["set_warmstart", "solve"]
    assert np.array_equal(f.calls[1][3], [[4.0, 5.0]])


def test_shim_stage_yref_forwards_the_rows_set():
    N = 5
    shim, f = _shim(True, N)
    rows = np.arange((N + 1) * 6, dtype=float).reshape(N + 1, 6)
    for i in range(N):
        shim.cost_set(i, "yref", rows[i])
    shim.cost_set(N, "yref", rows[N, :4])
    with pytest.raises(ValueError):
        shim.cost_set(N, "yref", rows[N])            # the terminal stage takes ny_e = 4 values
    shim.solve()
    assert [c[0] for c in f.calls] == ["set_reference", "set_warmstart", "solve"]
    want = rows.copy(); want[N, 4:] = 0.0
    assert np.array_equal(f.calls[0][1], want[None])
    assert np.array_equal(f.calls[2][3], [[1.0, 2.0]])     # the goal (slack schedule, bookkeeping) is the constructor's


def test_shim_stage_yref_starts_from_goal():
    shim, f = _shim(True)
    shim.solve()
    assert np.array_equal(f.calls[0][1][0], goal_rows(np.array([1.0, 2.0]), 5))


def test_stage_rows_clamp():
    y = np.arange(4 * 6, dtype=float).reshape(4, 6)
    R = stage_rows(y, 2, 3)
    assert np.array_equal(R[:2], y[2:4]) and np.array_equal(R[2], y[3]) and np.array_equal(R[3, :4], y[3, :4]) and (R[3, 4:] == 0).all()


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


def test_goal_reference_reproduces_export_qp(orc):
    """with the goal-derived reference the shifted gradient is export_qp's own, exactly"""
    from helpers import oracle_P, random_batch
    N, no = 8, 3
    cfg = orc.config(N, no, 0.8)
    x0, goal, obst = random_batch(1, no, seed=4)
    P = oracle_P(orc, cfg, obst)[0]
    rng = np.random.default_rng(2)
    X = rng.uniform(-4, 4, (N + 1, 5)); U = rng.uniform(-2, 2, (N, 2))
    q = orc.export_qp(cfg, x0[0], P, goal[0], X, U)
    assert np.array_equal(shift_gradient(cfg, q, goal[0], goal_rows(goal[0], N))["g"], q["g"])


def test_shifted_gradient_is_the_reference_gradient(orc):
    """the shifted QP gradient equals W (y - yref_i) formed directly, in export_qp's variable order (du_i, dx_{i+1})"""
    from helpers import oracle_P, random_batch
    N, no = 8, 3
    cfg = orc.config(N, no, 0.8)
    x0, goal, obst = random_batch(1, no, seed=5)
    P = oracle_P(orc, cfg, obst)[0]
    rng = np.random.default_rng(3)
    X = rng.uniform(-4, 4, (N + 1, 5)); U = rng.uniform(-2, 2, (N, 2))
    R = stage_rows(rng.uniform(-3, 3, (N + 4, 6)), 2, N)
    g = shift_gradient(cfg, orc.export_qp(cfg, x0[0], P, goal[0], X, U), goal[0], R)["g"]
    q = stage_gradient(cfg, X, U, R)
    want = np.concatenate([np.concatenate([q[i, :2], q[i + 1, 2:]]) for i in range(N)])
    # (export_qp's gradient also has the LM and obstacle-free parts only through q: its cost blocks are the LS gradient)
    assert np.abs(g - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
