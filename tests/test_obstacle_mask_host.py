"""Per-instance obstacle masks (mpc_set_obstacle_mask) without a GPU: the header and the ctypes mirror, the packing of the mask words, the Python
layer's shape checks, the new step flag, and the cut of an instance's present obstacles against the oracle's look-ahead of the reduced problem."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import random_batch
from obstacle_mask_cases import active_columns, draw_masks, groups, poison

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_obstacle_mask_api():
    h = open(os.path.join(ROOT, "include", "mpc_gpu.h")).read()
    assert re.search(r"int mpc_set_obstacle_mask\(mpc_handle \*h, int batch, const uint32_t \*mask\);", h)
    assert re.search(r"int mpc_set_obstacle_mask_dev\(mpc_handle \*h, const uint32_t \*d_mask\);", h)
    assert re.search(r"#define MPC_STEP_MARGIN_ALL 256\b", h)
    assert re.search(r"mpc_linearize_dev is NOT masked", h)      # the geometry outputs keep reporting every obstacle: stated
    assert re.search(r"#define MPC_ABI_VERSION 7\b", h)


def test_library_exports_and_mirror_binds(built):
    import mpc_gpu
    L = mpc_gpu._lib
    assert L.SYMBOLS["mpc_set_obstacle_mask"][1] == [C.c_void_p, C.c_int, C.c_void_p]
    assert L.SYMBOLS["mpc_set_obstacle_mask_dev"][1] == [C.c_void_p, C.c_void_p]
    lib = L.lib()
    w = np.ones(1, np.uint32)
    assert lib.mpc_set_obstacle_mask(None, 1, w.ctypes.data) == L.MPC_ERR_ARG
    assert b"null handle" in lib.mpc_last_error()
    assert lib.mpc_set_obstacle_mask_dev(None, None) == L.MPC_ERR_ARG


def test_margin_all_collides_with_no_flag(built):
    import mpc_gpu
    L = mpc_gpu._lib
    flags = {k: getattr(L, k) for k in dir(L) if k.startswith("STEP_")}
    assert flags["STEP_MARGIN_ALL"] == 256
    h = open(os.path.join(ROOT, "include", "mpc_gpu.h")).read()
    header = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define MPC_(STEP_\w+) (\d+)", h)}
    assert header == flags                                  # the mirror and the header agree, flag for flag
    vals = sorted(header.values())
    assert len(set(vals)) == len(vals) and all(v & (v - 1) == 0 for v in vals)      # distinct single bits


def test_pack_round_trips():
    from mpc_gpu import pack_obstacle_mask, unpack_obstacle_mask
    rng = np.random.default_rng(5)
    for no in (1, 3, 10, 31, 32):
        a = rng.random((9, no)) < 0.5
        a[0] = True; a[1] = False
        w = pack_obstacle_mask(a)
        assert w.dtype == np.uint32 and w.shape == (9,) and w.flags["C_CONTIGUOUS"]
        assert w[0] == (0xFFFFFFFF if no == 32 else (1 << no) - 1) and w[1] == 0
        assert np.array_equal(unpack_obstacle_mask(w, no), a)
    only31 = np.zeros((1, 32), bool); only31[0, 31] = True
    assert pack_obstacle_mask(only31)[0] == 0x80000000
    assert pack_obstacle_mask(np.array([[1, 0, 1]]))[0] == 5          # 0 / 1 integers are booleans
    for bad in (np.ones(3, bool), np.ones((2, 33), bool), np.ones((2, 0), bool), np.ones((2, 2, 2), bool), np.array([[2, 0]])):
        with pytest.raises(ValueError):
            pack_obstacle_mask(bad)


class _Bare:
    """a BatchedMpc without a handle: the shape checks of set_obstacle_mask run before any library call"""
    def __new__(cls, n_obst, max_batch):
        import mpc_gpu
        s = object.__new__(mpc_gpu.BatchedMpc)
        s.n_obst, s.max_batch, s._h = n_obst, max_batch, C.c_void_p()
        return s


def test_python_layer_shape_errors(built):
    s = _Bare(3, 4)
    for bad in (np.ones((4, 2), bool), np.ones((4, 4), bool), np.ones(3, bool), np.ones((5, 3), bool), np.ones((0, 3), bool)):
        with pytest.raises(ValueError):
            s.set_obstacle_mask(bad)

    class Dev:      # anything that is not a host array counts as a device tensor
        shape = (3,)
        dtype = "torch.int32"

        def is_contiguous(self):
            return True
    with pytest.raises(ValueError, match="device obstacle mask"):
        s.set_obstacle_mask(Dev())


def test_pipeline_slices(built):
    import mpc_gpu.pipeline as pl
    calls = []

    class Part:
        def set_obstacle_mask(self, a):
            calls.append(a)
    p = object.__new__(pl.PipelinedMpc)
    p.parts = [(0, 3, Part(), None), (3, 5, Part(), None)]
    words = np.arange(5, dtype=np.int32)
    p.set_obstacle_mask_dev(words)
    assert np.array_equal(calls[0], words[:3]) and np.array_equal(calls[1], words[3:])
    p.set_obstacle_mask_dev(None)
    assert calls[2] is None and calls[3] is None


def test_active_columns_is_the_reduced_problem(built):
    """cutting the present obstacles out of the look-ahead of the full problem is the look-ahead of the reduced problem: every obstacle's prediction is
    its own, so the oracle of count k can be asked about a masked instance"""
    from oracle import oracle as orc
    N, no, B = 20, 5, 12
    rng = np.random.default_rng(2)
    _, _, obst = random_batch(B, no, seed=9)
    act = draw_masks(rng, B, no)
    assert sorted(set(act.sum(axis=1))) == list(range(no + 1))          # every count 0 .. no occurs
    assert any(row.any() and not row[: row.sum()].all() for row in act)      # ... and not only prefixes
    cfg = orc.config(N, no, 0.1 * N)
    for b in range(B):
        k = int(act[b].sum())
        full = orc.predict_params(cfg, obst[b])
        cut = active_columns(full, act[b])
        assert cut.shape == (N + 1, k, 2)
        if k:
            want = orc.predict_params(orc.config(N, k, 0.1 * N), active_columns(obst[b], act[b]))
            assert np.array_equal(cut, want)
    g = groups(act)
    assert sorted(i for idx in g.values() for i in idx) == list(range(B))
    for key, idx in g.items():
        assert all(tuple(act[i].tolist()) == key for i in idx)
    bad = poison(obst, act, np.nan)
    assert np.isnan(bad[~act]).all() and np.array_equal(bad[act], obst[act])
    P = np.stack([orc.predict_params(cfg, o) for o in obst])
    badP = poison(P, act, np.inf)
    assert np.isinf(badP[:, :, :, 0][np.broadcast_to(~act[:, None, :], (B, N + 1, no))]).all()
    assert np.array_equal(badP[:, 3][act], P[:, 3][act])
