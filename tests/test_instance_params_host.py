"""Per-instance cost weights and per-obstacle radii (mpc_set_instance_params) without a GPU: the header and the ctypes mirror, NULL-handle refusals,
the Python layer's argument validation, and the numpy QP rewrite (instance_params_qp.retarget_qp) against the oracle where the oracle can speak."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from instance_params_qp import derived, draw_sets, hval, retarget_qp, stage_gradient

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_instance_params_api():
    h = open(os.path.join(ROOT, "include", "mpc_gpu.h")).read()
    assert re.search(r"int mpc_set_instance_params\(mpc_handle \*h, int batch, const double \*W, const double \*We, const double \*r_safe, const double \*r_hit\);", h)
    assert re.search(r"int mpc_set_instance_params_dev\(mpc_handle \*h, const double \*d_W, const double \*d_We, const double \*d_r_safe, const double \*d_r_hit\);", h)
    assert re.search(r"r_hit\[b\]\[j\] = r_safe\[b\]\[j\] - \(cfg\.r_safe - 1\.2\)", h)      # the default hit radius is documented
    assert re.search(r"#define MPC_ABI_VERSION 7\b", h)


def test_mirror_binds_instance_params_api(built):
    import mpc_gpu
    L = mpc_gpu._lib
    assert L.SYMBOLS["mpc_set_instance_params"][1] == [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    assert L.SYMBOLS["mpc_set_instance_params_dev"][1] == [C.c_void_p] * 5
    lib = L.lib()
    w = np.ones((1, 6))
    assert lib.mpc_set_instance_params(None, 1, w.ctypes.data, None, None, None) == L.MPC_ERR_ARG
    assert b"null handle" in lib.mpc_last_error()
    assert lib.mpc_set_instance_params_dev(None, None, None, None, None) == L.MPC_ERR_ARG


class _Bare:
    """a BatchedMpc without a handle: the array plumbing of set_instance_params runs before any library call"""
    def __new__(cls, n_obst, max_batch):
        import mpc_gpu
        s = object.__new__(mpc_gpu.BatchedMpc)
        s.n_obst, s.max_batch, s._h = n_obst, max_batch, C.c_void_p()
        return s


def test_python_layer_shapes(built):
    s = _Bare(3, 4)
    (W, We, r, rh), B = s._instance_arrays(np.ones((4, 6)), None, np.array([1.6, 2.0, 2.4, 3.0]), None)
    assert B == 4 and We is None and rh is None and W.shape == (4, 6)
    assert r.shape == (4, 3) and np.array_equal(r[:, 0], [1.6, 2.0, 2.4, 3.0]) and np.array_equal(r[:, 0], r[:, 2])      # (B,) = one radius per instance
    assert r.flags["C_CONTIGUOUS"] and r.dtype == np.float64
    (_, _, r2, _), _ = s._instance_arrays(None, None, np.full((2, 3), 2.0), np.full((2, 3), 0.8))
    assert r2.shape == (2, 3)
    for bad in (dict(W=np.ones((4, 5))), dict(We=np.ones((4, 6))), dict(r_safe=np.ones((4, 2))), dict(r_hit=np.ones((4, 3, 1))),
                dict(W=np.ones((4, 6)), We=np.ones((3, 4))), dict(W=np.ones(6))):
        kw = dict(W=None, We=None, r_safe=None, r_hit=None); kw.update(bad)
        with pytest.raises(ValueError):
            s._instance_arrays(**kw)
    with pytest.raises(ValueError, match="not both"):
        class Dev:      # anything that is not a host array counts as a device tensor
            shape = (4, 6)
        s.set_instance_params(W=np.ones((4, 6)), We=Dev())


def test_pipeline_slices(built):
    import mpc_gpu.pipeline as pl
    calls = []

    class Part:
        def set_instance_params(self, *a):
            calls.append(a)

    p = object.__new__(pl.PipelinedMpc)
    p.parts = [(0, 3, Part(), None), (3, 5, Part(), None)]
    W = np.arange(30.0).reshape(5, 6); r = np.arange(10.0).reshape(5, 2)
    p.set_instance_params_dev(W=W, r_safe=r)
    assert np.array_equal(calls[0][0], W[:3]) and np.array_equal(calls[1][0], W[3:]) and calls[0][1] is None and np.array_equal(calls[1][2], r[3:])
    calls.clear()
    p.set_instance_params_dev()
    assert calls == [(None, None, None, None)] * 2


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


def _qp_inputs(orc, N, no, seed):
    from helpers import oracle_P, random_batch
    cfg = orc.config(N, no, 0.1 * N)
    x0, goal, obst = random_batch(1, no, seed=seed)
    P = oracle_P(orc, cfg, obst)[0]
    rng = np.random.default_rng(seed)
    X = rng.uniform(-4, 4, (N + 1, 5)); U = rng.uniform(-2, 2, (N, 2))
    return cfg, x0[0], goal[0], P, X, U, rng


def _same_qp(a, b, tol=1e-12):
    for k in ("H", "g", "Aeq", "beq", "Cs", "hs", "zs", "Zs", "lb", "ub"):
        x, y = a[k], b[k]
        assert x.shape == y.shape, k
        fin = np.isfinite(y)
        assert np.array_equal(np.isfinite(x), fin), k
        assert np.array_equal(x[~fin], y[~fin]), k
        scale = max(1.0, np.abs(y[fin]).max()) if fin.any() else 1.0
        assert np.abs(x[fin] - y[fin]).max() <= tol * scale if fin.any() else True, (k, np.abs(x[fin] - y[fin]).max())


def test_default_parameters_reproduce_export_qp(orc):
    cfg, x0, goal, P, X, U, _ = _qp_inputs(orc, 8, 3, 4)
    q = orc.export_qp(cfg, x0, P, goal, X, U)
    W0 = [cfg.W[k] for k in range(6)]; We0 = [cfg.We[k] for k in range(4)]
    r = retarget_qp(cfg, q, W0, We0, cfg.r_safe)
    for k in q:
        assert np.array_equal(r[k], q[k]), k


def test_obstacle_rows_are_stage_major(orc):
    """hs holds |p - o_j|^2 - r_safe^2 of [stage 1..][obstacle] at the linearisation point, which is what retarget_qp relies on"""
    cfg, x0, goal, P, X, U, _ = _qp_inputs(orc, 6, 4, 9)
    q = orc.export_qp(cfg, x0, P, goal, X, U)
    want = hval(X, P, np.full(4, cfg.r_safe))[1:6].reshape(-1)      # stages 1 .. N - 1: the terminal stage's slack weight is zero, its rows are not exported
    assert q["hs"].shape == want.shape and np.abs(q["hs"] - want).max() <= 1e-12


@pytest.mark.parametrize("N,no,seed", [(8, 3, 5), (12, 5, 6), (6, 10, 7)])
def test_retarget_equals_export_of_a_config_with_those_values(orc, N, no, seed):
    """weights, and a radius that is uniform within the instance: the oracle can express both, and the rewritten default export equals the export
    of a config built with them, to the project's linearisation tolerance"""
    cfg, x0, goal, P, X, U, rng = _qp_inputs(orc, N, no, seed)
    q = orc.export_qp(cfg, x0, P, goal, X, U)
    W, We, r = draw_sets(rng, cfg, 3)
    for k in range(3):
        cfg_k = orc.config(N, no, 0.1 * N, W=list(W[k]), We=list(We[k]), r_safe=float(r[k]))
        _same_qp(retarget_qp(cfg, q, W[k], We[k], r[k]), orc.export_qp(cfg_k, x0, P, goal, X, U))


def test_per_obstacle_radii_move_only_their_rows(orc):
    cfg, x0, goal, P, X, U, rng = _qp_inputs(orc, 7, 3, 11)
    q = orc.export_qp(cfg, x0, P, goal, X, U)
    W0 = [cfg.W[k] for k in range(6)]; We0 = [cfg.We[k] for k in range(4)]
    rr = np.array([1.6, cfg.r_safe, 3.0])
    r = retarget_qp(cfg, q, W0, We0, rr)
    d = (r["hs"] - q["hs"]).reshape(6, 3)
    assert np.allclose(d[:, 0], cfg.r_safe ** 2 - 1.6 ** 2, rtol=0, atol=1e-12) and np.all(d[:, 1] == 0.0) and np.allclose(d[:, 2], cfg.r_safe ** 2 - 9.0, rtol=0, atol=1e-12)
    assert np.array_equal(r["Cs"], q["Cs"]) and np.array_equal(r["g"], q["g"]) and np.array_equal(r["H"], q["H"])
    assert np.abs(r["hs"] - hval(X, P, rr)[1:7].reshape(-1)).max() <= 1e-12


def test_gradient_and_diagonals_follow_the_weights(orc):
    cfg, x0, goal, P, X, U, rng = _qp_inputs(orc, 6, 3, 13)
    W, We, _ = draw_sets(rng, cfg, 1)
    q = retarget_qp(cfg, orc.export_qp(cfg, x0, P, goal, X, U), W[0], We[0], cfg.r_safe)
    g = stage_gradient(cfg, X, U, goal, W[0], We[0])
    want = np.concatenate([np.concatenate([g[i, :2], g[i + 1, 2:]]) for i in range(6)])
    assert np.abs(q["g"] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    hs, ht, _, _ = derived(cfg, W[0], We[0])
    assert np.array_equal(np.diag(q["H"])[:7], np.concatenate([hs[:2], hs[2:]])) and np.array_equal(np.diag(q["H"])[-5:], ht)
