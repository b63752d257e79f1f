"""mpc_create2: the creation entry point for 1..32 obstacles (beyond 10 with N <= 31).  Argument validation and the no-device path only: no
compute calls here (CPU suite)."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib(built):
    from mpc_gpu import _lib
    return _lib


def test_create2_is_exported_and_bound(lib):
    L = C.CDLL(lib.LIB_PATH)
    assert hasattr(L, "mpc_create2")
    assert "mpc_create2" in lib.SYMBOLS
    assert hasattr(lib.lib(), "mpc_create2")


@pytest.mark.parametrize("bad", [dict(n_obst=0), dict(n_obst=33), dict(N=1), dict(N=63), dict(N=32, n_obst=11), dict(N=40, n_obst=15)])
def test_create2_rejects_arguments_outside_its_range(lib, bad):
    L = lib.lib()
    cfg = lib.default_config(20, 15, 2.0)
    for k, v in bad.items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    assert L.mpc_create2(C.byref(cfg), 0, 1, C.byref(h)) == lib.MPC_ERR_ARG
    assert not h.value
    if bad.get("n_obst", 0) > 10 and bad.get("N", 0) > 31:
        assert b"N <= 31" in L.mpc_last_error()


@pytest.mark.parametrize("no", [11, 20, 32])
def test_create2_passes_validation_beyond_ten_obstacles(lib, no):
    L = lib.lib()
    cfg = lib.default_config(20, no, 2.0)
    h = C.c_void_p()
    rc = L.mpc_create2(C.byref(cfg), 0, 2, C.byref(h))
    if L.mpc_device_count() == 0:
        assert rc == lib.MPC_ERR_NODEVICE and b"no CPU path" in L.mpc_last_error()
    else:
        assert rc == lib.MPC_OK and h.value
        assert L.mpc_destroy(h) == lib.MPC_OK
    # mpc_create keeps its documented range
    assert L.mpc_create(C.byref(cfg), 0, 2, C.byref(C.c_void_p())) == lib.MPC_ERR_ARG


@pytest.mark.parametrize("N,no", [(10, 15), (30, 30), (31, 32)])
def test_default_config_matches_the_oracle_beyond_ten_obstacles(lib, N, no):
    from oracle import oracle as orc
    cfg = lib.default_config(N, no, 0.1 * N)
    o = orc.config(N, no, 0.1 * N)
    for name, _ in lib.MpcConfig._fields_:
        a, b = getattr(cfg, name), getattr(o, name)
        if hasattr(a, "__len__"):
            assert list(a) == list(b), name
        else:
            assert a == b, name
