"""Per-instance box bounds (mpc_set_instance_bounds) without a GPU: the header and the ctypes mirror, the packed table of the device form, the Python
layer's shape checks, the slicing of PipelinedMpc, and the draws the GPU tests use."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from instance_bounds_cases import DEFAULTS, as_cfg, draw_bounds, per_instance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_instance_bounds_api():
    h = open(os.path.join(ROOT, "include", "mpc_gpu.h")).read()
    assert re.search(r"int mpc_set_instance_bounds\(mpc_handle \*h, int batch, const double \*bx_lo, const double \*bx_hi,\s*const double \*bu_lo, "
                     r"const double \*bu_hi\);", h)
    assert re.search(r"int mpc_set_instance_bounds_dev\(mpc_handle \*h, const double \*d_bounds\);", h)
    assert re.search(r"#define MPC_ABI_VERSION 7\b", h)      # no struct and no existing signature changed


def test_library_exports_and_mirror_binds(built):
    import mpc_gpu
    L = mpc_gpu._lib
    raw = C.CDLL(L.LIB_PATH)
    for name in ("mpc_set_instance_bounds", "mpc_set_instance_bounds_dev"):
        assert hasattr(raw, name), f"{name} declared in include/mpc_gpu.h but not exported by libmpcgpu.so"
    assert L.SYMBOLS["mpc_set_instance_bounds"][1] == [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    assert L.SYMBOLS["mpc_set_instance_bounds_dev"][1] == [C.c_void_p, C.c_void_p]
    lib = L.lib()
    lo = -np.ones(2)
    assert lib.mpc_set_instance_bounds(None, 1, None, None, lo.ctypes.data, None) == L.MPC_ERR_ARG
    assert b"null handle" in lib.mpc_last_error()
    assert lib.mpc_set_instance_bounds_dev(None, None) == L.MPC_ERR_ARG
    assert lib.mpc_abi_version() == 7


def test_pack_order_broadcast_and_defaults(built):
    import mpc_gpu
    from mpc_gpu import pack_instance_bounds
    cfg = mpc_gpu.default_config(20, 3, 2.0)
    B = 5
    rng = np.random.default_rng(3)
    bx_lo, bx_hi = -rng.uniform(1, 2, (B, 4)), rng.uniform(1, 2, (B, 4))
    bu_lo, bu_hi = -rng.uniform(1, 2, (B, 2)), rng.uniform(1, 2, (B, 2))
    t = pack_instance_bounds(cfg, B, bx_lo, bx_hi, bu_lo, bu_hi)
    assert t.shape == (B, 12) and t.dtype == np.float64 and t.flags["C_CONTIGUOUS"]
    # row order: bu_lo[2], bu_hi[2], bx_lo[4], bx_hi[4]; bx in mpc_config's order
    assert np.array_equal(t[:, 0:2], bu_lo) and np.array_equal(t[:, 2:4], bu_hi)
    assert np.array_equal(t[:, 4:8], bx_lo) and np.array_equal(t[:, 8:12], bx_hi)
    # a missing group takes the config's value, in every row
    d = pack_instance_bounds(cfg, B)
    want = np.concatenate([DEFAULTS["bu_lo"], DEFAULTS["bu_hi"], DEFAULTS["bx_lo"], DEFAULTS["bx_hi"]])
    assert np.array_equal(d, np.tile(want, (B, 1)))
    only = pack_instance_bounds(cfg, B, bu_hi=bu_hi)
    assert np.array_equal(only[:, 2:4], bu_hi)
    assert np.array_equal(np.delete(only, [2, 3], axis=1), np.delete(d, [2, 3], axis=1))
    # ... the config's own, not the library's defaults
    cfg2 = mpc_gpu.default_config(20, 3, 2.0, bx_hi=[1.0, 2.0, 3.0, 4.0], bu_lo=[-0.5, -0.25])
    d2 = pack_instance_bounds(cfg2, 2)
    assert np.array_equal(d2[:, 8:12], [[1.0, 2.0, 3.0, 4.0]] * 2) and np.array_equal(d2[:, 0:2], [[-0.5, -0.25]] * 2)
    # a single row is broadcast to the batch
    one = pack_instance_bounds(cfg, B, bx_lo=bx_lo[0], bu_hi=[3.0, 4.0])
    assert np.array_equal(one[:, 4:8], np.tile(bx_lo[0], (B, 1))) and np.array_equal(one[:, 2:4], [[3.0, 4.0]] * B)
    for bad in (dict(bx_lo=np.zeros((B, 3))), dict(bu_lo=np.zeros((B + 1, 2))), dict(bx_hi=np.zeros(5)), dict(bu_hi=np.zeros((B, 2, 1)))):
        with pytest.raises(ValueError):
            pack_instance_bounds(cfg, B, **bad)


class _Bare:
    """a BatchedMpc without a handle: the shape checks run before any library call"""
    def __new__(cls, n_obst, max_batch):
        import mpc_gpu
        s = object.__new__(mpc_gpu.BatchedMpc)
        s.n_obst, s.max_batch, s._h = n_obst, max_batch, C.c_void_p()
        return s


def test_python_layer_shape_errors(built):
    s = _Bare(3, 4)
    for bad in (dict(bx_lo=np.zeros((4, 2))), dict(bu_lo=np.zeros((4, 4))), dict(bx_lo=np.zeros((4, 4)), bu_lo=np.zeros((3, 2))), dict(bu_hi=np.zeros(3))):
        with pytest.raises(ValueError):
            s.set_instance_bounds(**bad)

    class Dev:
        shape = (4, 11)
        dtype = "torch.float64"

        def is_contiguous(self):
            return True
    with pytest.raises(ValueError, match="device bounds table"):
        s.set_instance_bounds_dev(Dev())


def test_pipeline_slices(built):
    import mpc_gpu.pipeline as pl
    calls = []

    class Part:
        def set_instance_bounds(self, *a):
            calls.append(("host",) + a)

        def set_instance_bounds_dev(self, t):
            calls.append(("dev", t))
    p = object.__new__(pl.PipelinedMpc)
    p.parts = [(0, 3, Part(), None), (3, 5, Part(), None)]
    table = np.arange(60, dtype=np.float64).reshape(5, 12)
    p.set_instance_bounds_dev(table)
    assert np.array_equal(calls[0][1], table[:3]) and np.array_equal(calls[1][1], table[3:])
    p.set_instance_bounds_dev(None)
    assert calls[2] == ("dev", None) and calls[3] == ("dev", None)
    del calls[:]
    bx_hi = np.arange(20, dtype=np.float64).reshape(5, 4); bu_lo = np.array([-1.0, -2.0])
    p.set_instance_bounds(bx_hi=bx_hi, bu_lo=bu_lo)
    for (kind, a_bx_lo, a_bx_hi, a_bu_lo, a_bu_hi), (lo, hi) in zip(calls, ((0, 3), (3, 5))):
        assert kind == "host" and a_bx_lo is None and a_bu_hi is None
        assert np.array_equal(a_bx_hi, bx_hi[lo:hi]) and np.array_equal(a_bu_lo, bu_lo)      # rows are cut, a single row goes to every part
    del calls[:]
    p.set_instance_bounds()
    assert calls == [("host", None, None, None, None)] * 2


def test_draw_bounds():
    rng = np.random.default_rng(1223)
    menu, group = draw_bounds(rng, 16)
    assert len(menu) == 4 and sorted(group.tolist()) == sorted((np.arange(16) % 4).tolist())
    assert all(np.array_equal(menu[0][k], DEFAULTS[k]) for k in DEFAULTS)
    for e in menu[1:]:
        assert (e["bx_lo"] < 0).all() and (e["bx_hi"] > 0).all() and (e["bu_lo"] < 0).all() and (e["bu_hi"] > 0).all()
        assert (np.abs(e["bx_lo"][:2]) >= 6.5).all() and (e["bx_hi"][:2] <= 7.5).all()
        assert 0.8 <= e["bx_hi"][2] <= 3.0 and 1.0 <= -e["bx_lo"][3] <= 4.0 and (np.abs(e["bu_lo"]) >= 1.5).all() and (e["bu_hi"] <= 6.0).all()
        assert not np.array_equal(-e["bx_lo"], e["bx_hi"]) and not np.array_equal(-e["bu_lo"], e["bu_hi"])      # asymmetric
    arr = per_instance(menu, group)
    assert arr["bx_lo"].shape == (16, 4) and arr["bu_hi"].shape == (16, 2)
    assert all(np.array_equal(arr["bu_lo"][b], menu[group[b]]["bu_lo"]) for b in range(16))
    assert as_cfg(menu[1])["bx_hi"] == [float(x) for x in menu[1]["bx_hi"]]
