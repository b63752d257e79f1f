"""Per-seed trajectories of a seed sweep without a device: header, symbol table, ctypes struct and bindings agree on the two new entry points; the ABI
version and the refill's prototype stay; run_seed_sweep refuses bad trace arguments before any device call; the byte count against a hand-computed case;
sweep_record composes with visualisation_inputs on a synthetic trace."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import trace_cases as tc
from test_sweep_host import ROOT, header_prototype, header_text

START, GOAL = [-7.0, -7.0, np.pi / 4, 0, 0], [7.0, 7.0]


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
def test_header_and_symbol_table_agree_and_the_abi_version_stays():
    from mpc_gpu import _lib
    ctype = lambda t: (C.POINTER(_lib.EpisodeTrace) if "mpc_episode_trace" in t else _lib._vp) if t.endswith("*") else {"int": C.c_int, "unsigned": C.c_uint}[t]
    for name in tc.NEW:
        proto = header_prototype(name)
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and args == [ctype(t) for t, _ in proto], name
    assert [n for _, n in header_prototype("mpc_episode_trace_set_dev")] == ["h", "rows", "max_steps", "t"]
    assert [n for _, n in header_prototype("mpc_episode_trace_dev")][:3] == ["h", "slots", "phase"] and header_prototype("mpc_episode_trace_dev")[-1] == ("void *", "stream")
    hdr = header_text()
    assert int(re.search(r"#define\s+MPC_ABI_VERSION\s+(\d+)", hdr).group(1)) == 7 == _lib.ABI_VERSION
    assert len(header_prototype("mpc_episode_refill_dev")) == 26 and len(_lib.SYMBOLS["mpc_episode_refill_dev"][1]) == 26
    phases = {n: int(re.search(r"#define\s+MPC_TRACE_" + n + r"\s+(\d+)", hdr).group(1)) for n in ("START", "STEP")}
    assert phases == dict(START=_lib.TRACE_START, STEP=_lib.TRACE_STEP) == dict(START=0, STEP=1)


def test_ctypes_struct_and_header_agree_on_field_order_and_size():
    from mpc_gpu import _lib
    from mpc_gpu.solver import BatchedMpc
    src = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    body = re.search(r"typedef struct mpc_episode_trace\s*\{(.*?)\}\s*mpc_episode_trace\s*;", src, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            assert "*" in decl, decl                    # device pointers only
            fields += re.findall(r"\*\s*(\w+)", decl)
    assert fields == tc.TRACE_FIELDS == [n for n, _ in _lib.EpisodeTrace._fields_] == list(BatchedMpc.TRACE_FIELDS)
    assert all(t is C.c_void_p for _, t in _lib.EpisodeTrace._fields_)
    # the refill's own struct is untouched
    assert [n for n, _ in _lib.RefillTables._fields_] == ["W", "We", "r_safe", "r_hit", "mask", "bounds", "slot_W", "slot_We", "slot_r_safe", "slot_r_hit",
                                                          "slot_mask", "slot_bounds", "log", "res_log"]
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "mpc_gpu.h"\nint main(void) { printf("%zu %zu %zu %zu", '
                                                'sizeof(mpc_episode_trace), offsetof(mpc_episode_trace, len), offsetof(mpc_episode_trace, iters), '
                                                'offsetof(mpc_episode_trace, pred)); return 0; }\n')
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        size, off_len, off_iters, off_pred = map(int, subprocess.check_output([os.path.join(d, "s")]).split())
    T = _lib.EpisodeTrace
    assert size == C.sizeof(T) and off_len == T.len.offset and off_iters == T.iters.offset and off_pred == T.pred.offset


def test_bindings_hand_every_argument_to_its_position(monkeypatch):
    from mpc_gpu import _lib
    from mpc_gpu.solver import BatchedMpc
    seen = {}

    class Fake:
        def __getattr__(self, name):
            def call(*a):
                if name == "mpc_episode_trace_set_dev" and a[3] is not None:        # (the struct lives only during the call: copy it out)
                    a = a[:3] + ({n: getattr(a[3]._obj, n) for n in tc.TRACE_FIELDS},)
                seen[name] = a
                return 0
            return call
    monkeypatch.setattr(_lib, "lib", lambda: Fake())
    m = object.__new__(BatchedMpc)
    m._h = C.c_void_p(4096)
    py = lambda n: n[2:] if n.startswith("d_") else n
    try:
        proto = header_prototype("mpc_episode_trace_dev")
        vals = {n: 1000 + 8 * i for i, (t, n) in enumerate(proto) if t.endswith("*") and n != "h"}
        m.episode_trace_dev(slots=6, phase=1, **{py(n): v for n, v in vals.items()})
        got = seen["mpc_episode_trace_dev"]
        assert len(got) == len(proto)
        for (t, n), a in zip(proto, got):
            if n == "h":
                assert a.value == 4096
            elif t.endswith("*"):
                assert a.value == vals[n], n
            else:
                assert a == dict(slots=6, phase=1)[n], n
        vals = {n: 2000 + 8 * i for i, n in enumerate(tc.TRACE_FIELDS)}
        m.episode_trace_set_dev(5, 80, **vals)
        h, rows, max_steps, fields = seen["mpc_episode_trace_set_dev"]
        assert h.value == 4096 and (rows, max_steps) == (5, 80) and fields == vals
        m.episode_trace_set_dev(2, 7, **dict(vals, pred=None))
        assert seen["mpc_episode_trace_set_dev"][3] == dict(vals, pred=None)
        m.episode_trace_set_dev()                       # detach: rows 0, a null struct
        assert seen["mpc_episode_trace_set_dev"][1:] == (0, 0, None)
    finally:
        m._h = C.c_void_p()


# ---------------------------------------------------------------------------------------------------------------- 2. refusals before any device call
def test_trace_arguments_are_refused_before_any_device_call(ep, no_device):
    run = lambda **kw: ep.run_seed_sweep(START, GOAL, "RANDOM", (0, 10), 4, **kw)
    # wrong types
    for bad in ("all", 3, 2.5, {0, 4}, {0: 1}, [0.0, 4.0], [[0, 4]], [], [True, False], np.array([0.5]), (i for i in range(3)), b"\x01"):
        with pytest.raises(ValueError, match="trace"):
            run(trace=bad)
    # out of range (indices, not seeds: 0 .. count-1), duplicates
    for bad in ([0, 10], [-1], [3, 4, 12], range(5, 11), np.array([9, 10])):
        with pytest.raises(ValueError, match="trace.*outside"):
            run(trace=bad)
    with pytest.raises(ValueError, match="trace.*outside"):          # ... of THIS sweep: seed 37 of seeds 37 .. 46 is index 0
        ep.run_seed_sweep(START, GOAL, "RANDOM", (37, 10), 4, trace=[37])
    for bad in ([0, 4, 4], (9, 0, 9), np.array([1, 1])):
        with pytest.raises(ValueError, match="trace.*twice"):
            run(trace=bad)
    for kw in (dict(trace=True, trace_pred=1), dict(trace=True, trace_pred=None), dict(trace=[0], trace_pred="yes")):
        with pytest.raises(ValueError, match="trace_pred"):
            run(**kw)
    for kw in (dict(trace=True, trace_max_bytes=-1), dict(trace=True, trace_max_bytes=1e9), dict(trace=True, trace_max_bytes=None), dict(trace=True, trace_max_bytes=True)):
        with pytest.raises(ValueError, match="trace_max_bytes"):
            run(**kw)
    # the byte count: stated, with the way out
    need = ep.trace_bytes(10, 400, 20, 5, pred=True)
    with pytest.raises(ValueError, match=rf"trace.*{need} bytes.*fewer seeds.*trace_pred=False"):
        run(trace=True, trace_max_bytes=need - 1)
    small = ep.trace_bytes(10, 400, 20, 5, pred=False)
    with pytest.raises(ValueError, match=rf"{small} bytes.*fewer seeds") as e:
        run(trace=True, trace_pred=False, trace_max_bytes=small - 1)
    assert "trace_pred=False" not in str(e.value)
    need7 = ep.trace_bytes(2, 50, 10, 7, pred=True)                  # ... from rows, max_iter, N and n_obst as given
    with pytest.raises(ValueError, match=rf"{need7} bytes"):
        run(trace=[1, 8], max_iter=50, N=10, n_obst=7, trace_max_bytes=need7 - 1)
    # a valid trace passes the validation and is refused only by the fixture, behind it; so is no trace at all
    for kw in (dict(trace=True), dict(trace=[0, 4, 9]), dict(trace=range(10)), dict(trace=np.array([9, 0], dtype=np.uint8)), dict(trace=True, trace_max_bytes=need),
               dict(trace=None), dict(trace=False, trace_pred="ignored")):
        with pytest.raises(AssertionError, match="must not touch"):
            run(**kw)
    # still not offered: the keyword is `trace`, and `record` stays run_episodes'
    for kw in (dict(record=True), dict(record=True, trace=True), dict(record=True, trace=[0])):
        with pytest.raises(TypeError, match="record"):
            run(**kw)


def test_sweep_trace_is_normalised(ep):
    t = ep._sweep_trace(10, 400, 20, 5, trace=[9, 0, 4])
    assert t["seeds"].tolist() == [9, 0, 4] and t["seed_row"].dtype == np.int32 and t["seed_row"].tolist() == [1, -1, -1, -1, 2, -1, -1, -1, -1, 0]
    assert t["pred"] is True and t["bytes"] == ep.trace_bytes(3, 400, 20, 5)
    t = ep._sweep_trace(4, 12, 20, 5, trace=True, trace_pred=False)
    assert t["seeds"].tolist() == [0, 1, 2, 3] and t["seed_row"].tolist() == [0, 1, 2, 3] and t["pred"] is False
    assert ep._sweep_trace(4, 12, 20, 5) is None and ep._sweep_trace(4, 12, 20, 5, trace=False) is None


def test_byte_count_against_a_hand_computed_case(ep):
    import mpc_gpu
    c = tc.BYTES_CASE
    assert ep.trace_bytes(c["rows"], c["max_iter"], c["N"], c["n_obst"], pred=False) == c["without_pred"] == 7332
    assert ep.trace_bytes(c["rows"], c["max_iter"], c["N"], c["n_obst"], pred=True) == c["with_pred"] == 32532
    assert ep.trace_bytes(0, 400, 20, 5) == 0 and mpc_gpu.trace_bytes is ep.trace_bytes
    # the arrays run_seed_sweep allocates, element by element (float64 / int32)
    R, T, N, no = 7, 33, 12, 15
    elems64 = R * (T + 1) * 5 + R * (T + 1) * no * 4 + R * T * 2
    assert ep.trace_bytes(R, T, N, no, pred=False) == 8 * elems64 + 4 * (2 * R * T + R)
    assert ep.trace_bytes(R, T, N, no, pred=True) == 8 * (elems64 + R * T * (N + 1) * 5) + 4 * (2 * R * T + R)


# ---------------------------------------------------------------------------------------------------------------- 3. sweep_record
def test_sweep_record_and_visualisation_inputs_compose(ep):
    import mpc_gpu
    assert mpc_gpu.sweep_record is ep.sweep_record and "sweep_record" in mpc_gpu.__all__
    res = tc.synthetic_result(L=(4, 7), N=6, n_obst=2)
    for k, L in ((1, 4), (3, 7)):
        t = res["trace"][k]
        rec = ep.sweep_record(res, k)
        assert rec["simX"].shape == (L + 1, 1, 5) and rec["obst_traj"].shape == (L + 1, 1, 2, 4) and rec["pred"].shape == (L, 1, 7, 5)
        assert rec["table"].shape == (1, 6) and np.array_equal(rec["table"][0], res["table"][k]) and np.array_equal(rec["x_last"][0], res["x_last"][k])
        assert np.array_equal(rec["simX"][:, 0], t["simX"]) and np.array_equal(rec["obst_traj"][:, 0], t["obst_traj"]) and np.array_equal(rec["pred"][:, 0], t["pred"])
        v = ep.visualisation_inputs(rec, 0)
        assert v["trajectory"].shape == (2, L + 1) and np.array_equal(v["trajectory"], t["simX"][:, :2].T)
        assert len(v["obstacles"]) == 2 and all(np.array_equal(v["obstacles"][j], t["obst_traj"][:, j, :2].T) for j in range(2))
        # the solved horizon, re-assembled from the shifted iterate: row 0 zeros; row j + 1 = the state the solve started from, then stages 1 .. N
        assert v["pred"].shape == (L + 1, 7, 2) and not v["pred"][0].any()
        for j in range(L):
            assert np.array_equal(v["pred"][j + 1, 0], t["simX"][j, :2])
            assert np.array_equal(v["pred"][j + 1, 1:6], t["pred"][j, 0:5, :2]) and np.array_equal(v["pred"][j + 1, 6], t["pred"][j, 6, :2])
        # ... and it is what visualisation_inputs makes of the same seed recorded as column 2 of a batch of 3
        batch = dict(simX=np.repeat(rec["simX"], 3, axis=1), obst_traj=np.repeat(rec["obst_traj"], 3, axis=1), pred=np.repeat(rec["pred"], 3, axis=1),
                     table=np.repeat(rec["table"], 3, axis=0))
        w = ep.visualisation_inputs(batch, 2)
        assert np.array_equal(w["trajectory"], v["trajectory"]) and np.array_equal(w["pred"], v["pred"])


def test_sweep_record_refuses_clearly(ep):
    res = tc.synthetic_result()
    with pytest.raises(ValueError, match="not traced"):
        ep.sweep_record(res, 0)
    with pytest.raises(ValueError, match="not traced"):
        ep.sweep_record(res, 1.0)
    with pytest.raises(ValueError, match="without a trace"):
        ep.sweep_record({k: v for k, v in res.items() if k != "trace"}, 1)
    del res["trace"][3]["pred"]
    with pytest.raises(ValueError, match="trace_pred=False"):
        ep.sweep_record(res, 3)
    assert ep.sweep_record(res, 1)["pred"].shape[1] == 1            # (the other seed still has them)
