"""Per-seed sweep features without a device: header, symbol table, ctypes struct and bindings agree on the new entry points; run_seed_sweep refuses bad
per-seed arguments before any device call; the ring model on hand-made schedules."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from test_sweep_host import ROOT, header_prototype, header_text

START, GOAL = [-7.0, -7.0, np.pi / 4, 0, 0], [7.0, 7.0]
STRUCT_FIELDS = ["W", "We", "r_safe", "r_hit", "mask", "bounds", "slot_W", "slot_We", "slot_r_safe", "slot_r_hit", "slot_mask", "slot_bounds", "log", "res_log"]


@pytest.fixture
def ep():
    import mpc_gpu.episodes as ep
    return ep


@pytest.fixture
def no_device(monkeypatch):
    """any attempt to load the library or to create a handle fails the test"""
    from mpc_gpu import _lib
    from mpc_gpu.solver import BatchedMpc

    def touched(*a, **k):
        raise AssertionError("a refusal must not touch the device")
    monkeypatch.setattr(_lib, "lib", touched)
    monkeypatch.setattr(BatchedMpc, "__init__", touched)


# ---------------------------------------------------------------------------------------------------------------- 1. header, symbol table, struct, bindings
NEW = ("mpc_set_refill_tables_dev", "mpc_episode_status_log_dev", "mpc_episode_ring_dev", "mpc_episode_ring_fill_dev")


def test_header_and_symbol_table_agree_and_the_abi_version_stays():
    from mpc_gpu import _lib
    ctype = lambda t: (C.POINTER(_lib.RefillTables) if "mpc_refill_tables" in t else _lib._vp) if t.endswith("*") else {"int": C.c_int, "unsigned": C.c_uint}[t]
    for name in NEW:
        proto = header_prototype(name)
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and args == [ctype(t) for t, _ in proto], name
    assert int(re.search(r"#define\s+MPC_ABI_VERSION\s+(\d+)", header_text()).group(1)) == 7 == _lib.ABI_VERSION
    # the refill's own prototype is the pinned one: 26 arguments, the stream last
    assert len(header_prototype("mpc_episode_refill_dev")) == 26 and len(_lib.SYMBOLS["mpc_episode_refill_dev"][1]) == 26


def test_ctypes_struct_and_header_agree_on_field_order_and_size():
    from mpc_gpu import _lib
    src = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    body = re.search(r"typedef struct mpc_refill_tables\s*\{(.*?)\}\s*mpc_refill_tables\s*;", src, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            assert "*" in decl, decl                    # device pointers only
            fields += re.findall(r"\*\s*(\w+)", decl)
    assert fields == STRUCT_FIELDS == [n for n, _ in _lib.RefillTables._fields_]
    assert all(t is C.c_void_p for _, t in _lib.RefillTables._fields_)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "mpc_gpu.h"\nint main(void) { printf("%zu %zu %zu", '
                                                'sizeof(mpc_refill_tables), offsetof(mpc_refill_tables, slot_W), offsetof(mpc_refill_tables, res_log)); return 0; }\n')
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        size, off_slot, off_last = map(int, subprocess.check_output([os.path.join(d, "s")]).split())
    assert size == C.sizeof(_lib.RefillTables) and off_slot == _lib.RefillTables.slot_W.offset and off_last == _lib.RefillTables.res_log.offset


def test_bindings_hand_every_argument_to_its_position(monkeypatch):
    from mpc_gpu import _lib
    from mpc_gpu.solver import BatchedMpc
    seen = {}

    class Fake:
        def __getattr__(self, name):
            def call(*a):
                if name == "mpc_set_refill_tables_dev" and a[1] is not None:        # (the struct lives only during the call: copy it out)
                    a = (a[0], {n: getattr(a[1]._obj, n) for n in STRUCT_FIELDS})
                seen[name] = a
                return 0
            return call
    monkeypatch.setattr(_lib, "lib", lambda: Fake())
    m = object.__new__(BatchedMpc)
    m._h = C.c_void_p(4096)
    py = lambda n: n[2:] if n.startswith("d_") else n
    try:
        for name, method, ints in (("mpc_episode_status_log_dev", m.episode_status_log_dev, dict(slots=6)),
                                   ("mpc_episode_ring_dev", m.episode_ring_dev, dict(capacity=9)),
                                   ("mpc_episode_ring_fill_dev", m.episode_ring_fill_dev, dict(scenario="EDGE", seed_first=37, seed_count=10))):
            proto = header_prototype(name)
            vals = {n: 1000 + 8 * i for i, (t, n) in enumerate(proto) if t.endswith("*") and n not in ("h", "box")}
            method(**ints, **{py(n): v for n, v in vals.items()})
            got = seen[name]
            assert len(got) == len(proto)
            for (t, n), a in zip(proto, got):
                if n == "h":
                    assert a.value == 4096
                elif n == "box":
                    assert isinstance(a, C.c_void_p) and a.value
                elif t.endswith("*"):
                    assert a.value == vals[n], (name, n)
                else:
                    assert a == dict(ints, scenario=2)[n], (name, n)
        vals = {n: 2000 + 8 * i for i, n in enumerate(STRUCT_FIELDS)}
        m.set_refill_tables_dev(**vals)
        h, fields = seen["mpc_set_refill_tables_dev"]
        assert h.value == 4096 and fields == vals
        m.set_refill_tables_dev(W=7, slot_W=8)
        assert seen["mpc_set_refill_tables_dev"][1] == dict({n: None for n in STRUCT_FIELDS}, W=7, slot_W=8)
        m.set_refill_tables_dev()
        assert seen["mpc_set_refill_tables_dev"][1] is None
    finally:
        m._h = C.c_void_p()


def test_default_bounds_known_to_the_driver_are_the_library_s(built):
    from mpc_gpu import _lib, episodes
    cfg = _lib.default_config(20, 5, 2.0)
    assert {n: tuple(getattr(cfg, n)) for n in episodes.DEFAULT_BOUNDS} == episodes.DEFAULT_BOUNDS


# ---------------------------------------------------------------------------------------------------------------- 2. refusals before any device call
def test_per_seed_arguments_are_refused_before_any_device_call(ep, no_device):
    run = lambda **kw: ep.run_seed_sweep(START, GOAL, "RANDOM", (0, 10), 4, **kw)
    ok = np.full((10, 5), 2.0)
    bad = lambda v, at=(3, 1): (lambda a: (a.__setitem__(at, v), a)[1])(ok.copy())
    # wrong row counts
    for kw in (dict(r_safe=np.ones((9, 5))), dict(r_safe=np.ones(7)), dict(r_hit=np.ones((11, 5))), dict(W=np.ones((3, 6))), dict(We=np.ones((12, 4))),
               dict(active=np.ones((4, 5), dtype=bool)), dict(bounds=dict(bu_hi=np.ones((6, 2))))):
        with pytest.raises(ValueError, match="rows for 10 seeds"):
            run(**kw)
    # wrong widths
    for kw in (dict(r_safe=np.ones((10, 4))), dict(W=np.ones((10, 4))), dict(We=np.ones((10, 6))), dict(bounds=dict(bx_hi=np.ones((10, 2))))):
        with pytest.raises(ValueError):
            run(**kw)
    # a non-finite entry
    for kw in (dict(r_safe=bad(np.nan)), dict(r_hit=bad(np.inf)), dict(W=np.full((10, 6), np.nan)), dict(We=bad(np.inf)[:, :4]),
               dict(bounds=dict(bu_hi=bad(np.nan)[:, :2])), dict(bounds=dict(bx_lo=bad(-np.inf)[:, :4]))):
        with pytest.raises(ValueError, match="finite"):
            run(**kw)
    # a radius <= 0, a weight < 0 (a weight of 0 is valid and passes this check: it is refused only by the fixture, behind the validation)
    for kw in (dict(r_safe=bad(0.0)), dict(r_safe=bad(-1.0)), dict(r_hit=bad(0.0)), dict(W=np.full((10, 6), -1e-9)), dict(We=bad(-2.0)[:, :4])):
        with pytest.raises(ValueError, match="finite and"):
            run(**kw)
    with pytest.raises(AssertionError, match="must not touch"):
        run(W=np.zeros((10, 6)))
    # lo >= hi: both sides given; one side given, against the handle's value (bu -8 .. 8, bx -7 .. 7 / -10 .. 10)
    for b in (dict(bu_lo=[1.0, 1.0], bu_hi=[1.0, 2.0]), dict(bu_hi=np.full((10, 2), -8.0)), dict(bu_lo=bad(8.0)[:, :2]), dict(bx_hi=[7.0, 7.0, -10.0, 10.0]),
              dict(bx_lo=bad(7.5)[:, :4])):
        with pytest.raises(ValueError, match="must be below"):
            run(bounds=b)
    with pytest.raises(ValueError, match="must be below"):      # ... and against a handle value the caller overrides
        run(bounds=dict(bu_hi=[3.0, 3.0]), bu_lo=(3.0, 3.0))
    with pytest.raises(ValueError, match="keys"):
        run(bounds=dict(bz_hi=[1.0, 1.0]))
    # a mask bit at or above n_obst
    with pytest.raises(ValueError, match="n_obst"):
        run(active=np.ones((10, 6), dtype=bool))
    with pytest.raises(ValueError, match="n_obst"):
        run(active=np.ones((10, 5), dtype=bool), n_obst=4)
    # the ring
    for kw in (dict(ring=0), dict(ring=-3), dict(ring=2.5), dict(ring=True)):
        with pytest.raises(ValueError, match="ring"):
            run(**kw)
    for kw in (dict(ring=4, ring_every=0), dict(ring_every=-1), dict(ring=4, ring_every=1.5)):
        with pytest.raises(ValueError, match="ring_every"):
            run(**kw)
    # still not offered
    for kw in (dict(record=True), dict(record=True, status_log=True), dict(noise="torch"), dict(compact_from=64)):
        with pytest.raises(TypeError):
            run(**kw)


def test_sweep_features_are_normalised(ep):
    ft = ep._sweep_features(3, 5, ep.DEFAULT_BOUNDS, r_safe=[2.0, 2.5, 3.0], active=[[1, 0, 1, 1, 1]] * 3, bounds=dict(bu_hi=[4.0, 5.0]), ring=7, poll_every=25)
    assert ft["r_safe"].shape == (3, 5) and (ft["r_safe"][1] == 2.5).all() and ft["r_hit"] is None and ft["W"] is None
    assert ft["mask"].dtype == np.int32 and ft["mask"].tolist() == [0b11101] * 3
    assert ft["bounds"].shape == (3, 12) and ft["bounds"][2].tolist() == [-8, -8, 4, 5, -7, -7, -10, -10, 7, 7, 10, 10]
    assert ft["ring"] == 7 and ft["ring_every"] == 25 and ft["status_log"] is False
    assert ep._sweep_features(3, 5, ep.DEFAULT_BOUNDS, ring_every=4)["ring"] is None


# ---------------------------------------------------------------------------------------------------------------- 3. the ring model
def test_ring_model_capacity_at_least_the_count_gives_all_hits(ep):
    start = ep.refill_schedule([7, 3, 9, 4, 4, 6, 2, 8, 5, 5], 4)["start"]
    for cap in (10, 11, 64):
        for every in (1, 5, 25):
            assert ep.ring_model(start, cap, every).tolist() == [1] * 10


def test_ring_model_capacity_one_with_four_slots(ep):
    """lengths 3, 5, 5, 5 then 4, 4: starts 0 0 0 0 | 3 | 5 5 5 | 7 | 9 ...; the ring holds ONE index, the lowest not started at the last fill"""
    start = ep.refill_schedule([3, 5, 5, 5, 4, 4, 4, 4, 2, 2], 4)["start"]
    assert start.tolist() == [0, 0, 0, 0, 3, 5, 5, 5, 7, 9]
    # filled every step: in front of step t the entry holds handed(t); the first of the seeds that start at t hits, the others miss
    assert ep.ring_model(start, 1, 1).tolist() == [1, 0, 0, 0, 1, 1, 0, 0, 1, 1]
    # filled at steps 0, 4, 8: fill 0 holds seed 0; fill 4 (4 seeds started before step 4: 0 .. 3) holds seed 4, which started at 3 < 4 -- served by fill 0?  no:
    # its last fill is step 0, which held only k < 0 + 1.  Seed 5 starts at 5, last fill 4, handed(4) = 5 (seeds 0 .. 4) -> holds 5: hit.  Seed 8 starts at 7,
    # last fill 4: miss.  Seed 9 starts at 9, last fill 8, handed(8) = 9: hit
    assert ep.ring_model(start, 1, 4).tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 0, 1]
    # the inequality itself, entry by entry
    for cap, every in ((1, 1), (1, 4), (2, 3), (3, 25)):
        got = ep.ring_model(start, cap, every)
        for k, t in enumerate(start):
            t_f = (t // every) * every
            assert got[k] == int(k < int((start < t_f).sum()) + cap), (cap, every, k)


def test_ring_model_refuses_nonsense(ep):
    for a, cap, every in (([0, 0, 3], 0, 1), ([0, 0, 3], 1, 0), ([[0, 1]], 1, 1), ([0, -1], 1, 1)):
        with pytest.raises(ValueError):
            ep.ring_model(a, cap, every)
