"""The per-group record of multi-start episodes without a device: header, symbol table, ctypes struct and bindings agree on the two entry points and the
struct; the ABI version, the group step's and the group refill's prototypes and mpc_group_step_out stay; the numpy restatement of both phases
(multistart_record_cases) on made-up group words, held to what the header says by hand; run_multistart_episodes refuses bad record arguments before any device
use; the byte count against a hand-computed case; multistart_record composes with visualisation_inputs on a synthetic record."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import multistart_record_cases as rc
from test_sweep_host import ROOT, header_prototype, header_text


# ---------------------------------------------------------------------------------------------------------------- 1. header, symbol table, struct, bindings
def _ctype(t):
    from mpc_gpu import _lib
    if t.endswith("*"):
        return C.POINTER(_lib.GroupRecord) if "mpc_group_record" in t else (C.POINTER(_lib.GroupStepOut) if "mpc_group_step_out" in t else _lib._vp)
    return {"int": C.c_int, "unsigned": C.c_uint, "double": C.c_double}[t]


def test_header_and_symbol_table_agree_and_the_abi_version_stays():
    from mpc_gpu import _lib
    for name in rc.NEW:
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and args == [_ctype(t) for t, _ in header_prototype(name)], name
    assert [n for _, n in header_prototype("mpc_group_record_set_dev")] == ["h", "rows", "max_steps", "K", "r"]
    assert [n for _, n in header_prototype("mpc_group_record_dev")] == ["h", "groups", "K", "phase", "d_x", "d_obst", "d_X", "d_key", "d_status", "d_iters", "d_u0",
                                                                         "out", "stream"]
    assert [t for t, _ in header_prototype("mpc_group_record_dev")][4:] == ["const double *"] * 4 + ["const int32_t *"] * 2 + ["const double *",
                                                                                                                               "const mpc_group_step_out *", "void *"]
    hdr = header_text()
    assert int(re.search(r"#define\s+MPC_ABI_VERSION\s+(\d+)", hdr).group(1)) == 7 == _lib.ABI_VERSION
    phases = {n: int(re.search(r"#define\s+MPC_GROUP_RECORD_" + n + r"\s+(\d+)", hdr).group(1)) for n in ("SOLVED", "STEPPED")}
    assert phases == dict(SOLVED=_lib.GROUP_RECORD_SOLVED, STEPPED=_lib.GROUP_RECORD_STEPPED) == dict(SOLVED=rc.SOLVED, STEPPED=rc.STEPPED) == dict(SOLVED=0, STEPPED=1)
    # what was there stays: the group step, the group refill and the struct the record's second entry point shares with the group step
    step = header_prototype("mpc_group_step_dev")
    assert [n for _, n in step] == ["h", "groups", "K", "d_key", "d_status", "d_u0", "incumbent_margin", "flags", "d_x", "d_obst", "d_goal", "d_offsets", "d_noise",
                                    "randomness", "vmax", "d_X", "d_U", "out", "stream"]
    assert _lib.SYMBOLS["mpc_group_step_dev"][1] == [_ctype(t) for t, _ in step]
    refill = header_prototype("mpc_group_refill_dev")
    assert [n for _, n in refill] == ["h", "groups", "K", "scenario", "seed_first", "seed_count", "max_steps", "box", "d_start", "d_goal_rows", "per_seed", "d_offsets",
                                      "a", "stream"] and len(_lib.SYMBOLS["mpc_group_refill_dev"][1]) == 14
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    body = re.search(r"typedef struct mpc_group_step_out\s*\{(.*?)\}\s*mpc_group_step_out\s*;", src, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+)", body) == [n for n, _ in _lib.GroupStepOut._fields_] == ["winner", "best_key", "best_u0", "min_margin", "ep_flags", "ep_steps",
                                                                                            "lost", "switched", "member_x", "member_obst", "member_goal", "member_flags"]


def test_ctypes_struct_and_header_agree_on_field_order_size_and_offsets():
    from mpc_gpu import _lib
    from mpc_gpu.solver import BatchedMpc
    src = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    body = re.search(r"typedef struct mpc_group_record\s*\{(.*?)\}\s*mpc_group_record\s*;", src, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            assert "*" in decl, decl                    # device pointers only
            fields += re.findall(r"\*\s*(\w+)", decl)
    assert fields == rc.FIELDS == [n for n, _ in _lib.GroupRecord._fields_] == list(BatchedMpc.GROUP_RECORD_FIELDS)
    assert fields[2:] == list(rc.ARRAYS)[1:] and fields[1] == "len"          # the restatement is over the struct's arrays
    assert all(t is C.c_void_p for _, t in _lib.GroupRecord._fields_)
    with tempfile.TemporaryDirectory() as d:
        probe = ", ".join(f"offsetof(mpc_group_record, {n})" for n in fields)
        open(os.path.join(d, "s.c"), "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "mpc_gpu.h"\nint main(void) { size_t v[] = {sizeof(mpc_group_record), '
                                                + probe + '}; for (unsigned i = 0; i < sizeof v / sizeof v[0]; i++) printf("%zu ", v[i]); return 0; }\n')
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        got = list(map(int, subprocess.check_output([os.path.join(d, "s")]).split()))
    T = _lib.GroupRecord
    assert got == [C.sizeof(T)] + [getattr(T, n).offset for n in fields]


def test_bindings_hand_every_argument_to_its_position(monkeypatch):
    from mpc_gpu import _lib
    from mpc_gpu.solver import BatchedMpc
    seen = {}

    class Fake:
        def __getattr__(self, name):
            def call(*a):
                if name == "mpc_group_record_set_dev" and a[4] is not None:         # (the struct lives only during the call: copy it out)
                    a = a[:4] + ({n: getattr(a[4]._obj, n) for n in rc.FIELDS},)
                if name == "mpc_group_record_dev" and a[11] is not None:
                    a = a[:11] + (a[11]._obj,) + a[12:]
                seen[name] = a
                return 0
            return call
    monkeypatch.setattr(_lib, "lib", lambda: Fake())
    m = object.__new__(BatchedMpc)
    m._h = C.c_void_p(4096)
    py = lambda n: n[2:] if n.startswith("d_") else n
    try:
        proto = header_prototype("mpc_group_record_dev")
        out = _lib.GroupStepOut(winner=77)
        vals = {n: 1000 + 8 * i for i, (t, n) in enumerate(proto) if t.endswith("*") and n not in ("h", "out")}
        m.group_record_dev(groups=6, K=3, phase=1, out=out, **{py(n): v for n, v in vals.items()})
        got = seen["mpc_group_record_dev"]
        assert len(got) == len(proto)
        for (t, n), a in zip(proto, got):
            if n == "h":
                assert a.value == 4096
            elif n == "out":
                assert a is out
            elif t.endswith("*"):
                assert a.value == vals[n], n
            else:
                assert a == dict(groups=6, K=3, phase=1)[n], n
        vals = {n: 2000 + 8 * i for i, n in enumerate(rc.FIELDS)}
        m.group_record_set_dev(5, 80, 3, **vals)
        h, rows, max_steps, K, fields = seen["mpc_group_record_set_dev"]
        assert h.value == 4096 and (rows, max_steps, K) == (5, 80, 3) and fields == vals
        m.group_record_set_dev(2, 7, 64, **dict(vals, cand_X=None))
        assert seen["mpc_group_record_set_dev"][4] == dict(vals, cand_X=None)
        m.group_record_set_dev()                        # detach: rows 0, a null struct
        assert seen["mpc_group_record_set_dev"][1:] == (0, 0, 0, None)
    finally:
        m._h = C.c_void_p()


def test_the_group_drivers_lease_knows_how_to_undo_the_attach():
    from mpc_gpu.episodes import _HandleLease
    from mpc_gpu.multistart import MultiStartMpc, _group_lease
    assert callable(MultiStartMpc.group_record_set_dev) and callable(MultiStartMpc.group_record_off)
    calls = []

    class Fake:
        def group_record_set_dev(self, rows=0, max_steps=0, **kw):
            calls.append((rows, max_steps, sorted(kw)))

        def set_sqp(self, *a):
            calls.append(("set_sqp", a))
    lease = _group_lease(Fake(), None)
    assert isinstance(lease, _HandleLease) and lease.OFF == dict(_HandleLease.OFF, group_record_set_dev=(0,)) and "group_record_set_dev" not in _HandleLease.OFF
    with pytest.raises(RuntimeError):
        with lease:
            lease.attach("set_sqp", 2, 0.0)
            lease.attach("group_record_set_dev", 3, 9, len=1)
            raise RuntimeError("the block fails")
    assert calls == [("set_sqp", (2, 0.0)), (3, 9, ["len"]), (0, 0, []), ("set_sqp", ())]          # undone in reverse order, on an exception too


# ---------------------------------------------------------------------------------------------------------------- 2. the restatement on made-up group words
def _one_step(roles, T, K, N=3, no=2, seed=0):
    rng = np.random.default_rng(seed)
    inp, group_row, rec0 = rc.made_up(roles, T, K, N, no, rng)
    rec1 = rc.solved(rec0, group_row, T, inp, K)
    after = rc.fake_tail(inp, roles, K, rng)
    rec2 = rc.stepped(rec1, group_row, T, after, K)
    return inp, after, group_row, rec0, rec1, rec2


def _row_untouched(a, b, r):
    return all(np.array_equal(a[n][r], b[n][r]) for n in a)


@pytest.mark.parametrize("K", [1, 3, 64])
def test_both_phases_on_every_role_a_group_can_be_in(K):
    T = 5
    roles = ["run", "idle", "reach", "budget", "unrec", "run"]
    inp, after, row, rec0, rec1, rec2 = _one_step(roles, T, K, seed=K)
    R = rec0["len"].shape[0]
    assert R == 6 and row.tolist() == [5, 4, 3, 2, -1, 1], "the case itself: permuted rows, an unrecorded group, a row nobody owns"
    spare = (set(range(R)) - set(row.tolist())).pop()
    for g, role in enumerate(roles):
        r, m = row[g], slice(g * K, (g + 1) * K)
        if role == "unrec":
            continue
        if role == "idle":                              # a group that was idle on entry: neither phase writes a word of its row
            assert inp["ep_flags"][g] & 1 and _row_untouched(rec0, rec2, r)
            continue
        t = int(inp["ep_steps"][g])
        assert t == dict(run=1, reach=T - 2, budget=T - 1)[role] and rec0["len"][r] == t
        # SOLVED: the states the solve started from and the K candidates, at row t -- and nothing else
        assert np.array_equal(rec1["x"][r, t], inp["x"][g]) and np.array_equal(rec1["obst"][r, t], inp["obst"][g])
        assert np.array_equal(rec1["cand_key"][r, t], inp["key"][m]) and np.array_equal(rec1["cand_status"][r, t], inp["status"][m])
        assert np.array_equal(rec1["cand_iters"][r, t], inp["iters"][m]) and np.array_equal(rec1["cand_u0"][r, t], inp["u0"][m])
        assert np.array_equal(rec1["cand_X"][r, t], inp["X"][m]) and not np.array_equal(after["X"][m], inp["X"][m])      # the SOLVED plans, which the tail overwrote
        assert rec1["len"][r] == t and (rec1["winner"][r] == rc.I_SENT).all() and (rec1["u"][r] == rc.F_SENT).all() and (rec1["best_key"][r] == rc.F_SENT).all()
        others = np.ones(T + 1, bool); others[t] = False
        assert (rec1["x"][r][others] == rc.F_SENT).all() and (rec1["cand_X"][r][others[:T]] == rc.F_SENT).all() and (rec1["cand_key"][r][others[:T]] == rc.F_SENT).all()
        # STEPPED: winner, key, input at row t; the states it was left in at row `now`; len last
        now = t + 1
        assert after["ep_steps"][g] + (after["ep_flags"][g] & 1) == now
        assert (after["ep_flags"][g] & 1) == (role == "reach") and after["ep_steps"][g] == (t if role == "reach" else t + 1)
        assert rec2["winner"][r, t] == after["winner"][g] and rec2["best_key"][r, t] == after["best_key"][g] and np.array_equal(rec2["u"][r, t], after["best_u0"][g])
        assert np.array_equal(rec2["x"][r, now], after["x"][g]) and np.array_equal(rec2["obst"][r, now], after["obst"][g]) and rec2["len"][r] == now
        assert np.array_equal(rec2["x"][r, t], inp["x"][g]) and np.array_equal(rec2["cand_X"][r, t], inp["X"][m])        # what SOLVED wrote stays
        others[now] = False
        assert (rec2["x"][r][others] == rc.F_SENT).all() and (rec2["winner"][r][others[:T]] == rc.I_SENT).all()
        if role == "budget":
            assert now == T and after["ep_steps"][g] == T                                                            # the last row of the arrays is filled
    assert _row_untouched(rec0, rec2, spare)            # the unrecorded group wrote nowhere: the row nobody owns holds its sentinels
    assert any(after["winner"][g] == -1 and (after["best_u0"][g] == 0).all() for g in range(6) if roles[g] != "idle")      # a lost step is among them
    # a second STEPPED launch, and a SOLVED launch on a group that has just finished, write nothing
    assert all(np.array_equal(rc.stepped(rec2, row, T, after, K)[n], rec2[n]) for n in rec2)
    again = rc.solved(rec2, row, T, after, K)
    for g, role in enumerate(roles):
        if role in ("reach", "budget", "idle"):         # finished by the flag, or by the budget (t = T has no row)
            assert _row_untouched(rec2, again, row[g]), role


def test_the_restatement_without_plans_and_with_a_row_map_that_names_no_row():
    roles = ["run", "reach"]
    rng = np.random.default_rng(9)
    inp, row, rec = rc.made_up(roles, 4, 2, 3, 1, rng)
    del rec["cand_X"]
    one = rc.solved(rec, row, 4, inp, 2)
    assert "cand_X" not in one and np.array_equal(one["cand_key"][row[0], 1], inp["key"][0:2])
    for bad in (np.array([-1, -1], np.int32), np.array([rec["len"].shape[0], -1], np.int32)):          # not recorded; a row the arrays do not have
        for phase in (rc.solved, rc.stepped):
            out = phase(rec, bad, 4, inp, 2)
            assert all(np.array_equal(out[n], rec[n]) for n in rec)


# ---------------------------------------------------------------------------------------------------------------- 3. refusals before any device use
START, GOAL = np.tile([-7.0, -7.0, np.pi / 4, 0.0, 0.0], (6, 1)), [7.0, 7.0]


@pytest.fixture
def no_handle(monkeypatch):
    from mpc_gpu import multistart as ms

    def touched(*a, **k):
        raise AssertionError("a handle was made before the arguments were checked")
    monkeypatch.setattr(ms, "MultiStartMpc", type("Refuse", (), {"__init__": touched}))
    return ms


def test_record_arguments_are_refused_before_any_device_use(no_handle):
    ms = no_handle
    run = lambda **kw: ms.run_multistart_episodes(START, GOAL, "RANDOM", **kw)
    for bad in ("all", 3, 2.5, {0, 4}, {0: 1}, [0.0, 4.0], [[0, 4]], [], [True, False], np.array([0.5]), (i for i in range(3)), b"\x01", frozenset([1])):
        with pytest.raises(ValueError, match="record"):
            run(record=bad)
    for bad in ([0, 6], [-1], [3, 4, 12], range(2, 8), np.array([5, 6])):
        with pytest.raises(ValueError, match="record.*outside"):
            run(record=bad)
    for bad in ([0, 4, 4], (5, 0, 5), np.array([1, 1])):
        with pytest.raises(ValueError, match="record.*twice"):
            run(record=bad)
    for kw in (dict(record=True, record_plans=1), dict(record=True, record_plans=None), dict(record=[0], record_plans="yes")):
        with pytest.raises(ValueError, match="record_plans"):
            run(**kw)
    for kw in (dict(record=True, record_max_bytes=-1), dict(record=True, record_max_bytes=1e9), dict(record=True, record_max_bytes=None),
               dict(record=True, record_max_bytes=True)):
        with pytest.raises(ValueError, match="record_max_bytes"):
            run(**kw)
    # the byte count: stated, with the way out; K is that of the offsets given
    need = ms.group_record_bytes(6, 400, 20, 5, 5, plans=True)
    with pytest.raises(ValueError, match=rf"record.*{need} bytes.*fewer groups.*record_plans=False"):
        run(record=True, record_max_bytes=need - 1)
    small = ms.group_record_bytes(6, 400, 20, 5, 5, plans=False)
    with pytest.raises(ValueError, match=rf"{small} bytes.*fewer groups") as e:
        run(record=True, record_plans=False, record_max_bytes=small - 1)
    assert "record_plans=False" not in str(e.value)
    need7 = ms.group_record_bytes(2, 50, 10, 7, 3, plans=True)
    with pytest.raises(ValueError, match=rf"{need7} bytes"):
        run(record=[1, 4], max_iter=50, N=10, n_obst=7, offsets=(0.0, 2.5, -2.5), record_max_bytes=need7 - 1)
    # a valid record passes the validation and is refused only by the fixture, behind it; so is no record at all
    for kw in (dict(record=True), dict(record=[0, 4, 5]), dict(record=range(6)), dict(record=np.array([5, 0], dtype=np.uint8)), dict(record=True, record_max_bytes=need),
               dict(record=None), dict(record=False, record_plans="ignored")):
        with pytest.raises(AssertionError, match="before the arguments were checked"):
            run(**kw)
    # a sweep of groups still takes none
    for kw in (dict(record=True), dict(record=[0])):
        with pytest.raises(TypeError, match="record"):
            ms.run_multistart_sweep(START[0], GOAL, "RANDOM", (0, 6), 2, **kw)


def test_group_record_is_normalised():
    from mpc_gpu import multistart as ms
    t = ms._group_record(6, 400, 20, 5, 3, record=[5, 0, 4])
    assert t["groups"].tolist() == [5, 0, 4] and t["group_row"].dtype == np.int32 and t["group_row"].tolist() == [1, -1, -1, -1, 2, 0]
    assert t["plans"] is True and t["bytes"] == ms.group_record_bytes(3, 400, 20, 5, 3)
    t = ms._group_record(4, 12, 20, 5, 2, record=True, record_plans=False)
    assert t["groups"].tolist() == [0, 1, 2, 3] and t["group_row"].tolist() == [0, 1, 2, 3] and t["plans"] is False
    assert ms._group_record(4, 12, 20, 5, 2) is None and ms._group_record(4, 12, 20, 5, 2, record=False) is None


def test_byte_count_against_a_hand_computed_case():
    import mpc_gpu
    from mpc_gpu import multistart as ms
    c = rc.BYTES_CASE
    assert ms.group_record_bytes(c["rows"], c["max_iter"], c["N"], c["n_obst"], c["K"], plans=False) == c["without_plans"] == 6888
    assert ms.group_record_bytes(c["rows"], c["max_iter"], c["N"], c["n_obst"], c["K"], plans=True) == c["with_plans"] == 57288
    assert ms.group_record_bytes(0, 400, 20, 5, 3) == 0 and mpc_gpu.group_record_bytes is ms.group_record_bytes and "group_record_bytes" in mpc_gpu.__all__
    # the arrays of the restatement, element by element
    R, T, N, no, K = 7, 33, 12, 15, 5
    for plans in (True, False):
        rec = rc.empty_record(R, T, K, N, no, plans=plans)
        assert ms.group_record_bytes(R, T, N, no, K, plans=plans) == sum(a.nbytes for a in rec.values())


# ---------------------------------------------------------------------------------------------------------------- 4. multistart_record
def test_multistart_record_and_visualisation_inputs_compose():
    import mpc_gpu
    from mpc_gpu import multistart as ms
    from mpc_gpu.episodes import visualisation_inputs
    assert mpc_gpu.multistart_record is ms.multistart_record and "multistart_record" in mpc_gpu.__all__
    res = rc.synthetic_result(L=(4, 7), N=6, n_obst=2, K=3)
    for g, L in ((1, 4), (3, 7)):
        t = res["record"][g]
        rec = ms.multistart_record(res, g)
        assert rec["simX"].shape == (L + 1, 1, 5) and rec["obst_traj"].shape == (L + 1, 1, 2, 4) and rec["pred"].shape == (L, 1, 7, 5)
        assert rec["table"].shape == (1, 6) and np.array_equal(rec["table"][0], res["table"][g]) and np.array_equal(rec["x_last"][0], res["x_last"][g])
        assert np.array_equal(rec["simX"][:, 0], t["simX"]) and np.array_equal(rec["obst_traj"][:, 0], t["obst_traj"])
        v = visualisation_inputs(rec, 0)
        assert v["trajectory"].shape == (2, L + 1) and np.array_equal(v["trajectory"], t["simX"][:, :2].T)
        assert len(v["obstacles"]) == 2 and all(np.array_equal(v["obstacles"][j], t["obst_traj"][:, j, :2].T) for j in range(2))
        assert v["pred"].shape == (L + 1, 7, 2) and not v["pred"][0].any()
        for j in range(L):                              # the re-assembled horizon of step j is the SOLVED plan of its winner; of member 0 on a lost step
            w = int(t["winner"][j])
            assert np.array_equal(v["pred"][j + 1], t["cand_X"][j, max(w, 0)][:, :2]), (g, j)
            # the shifted layout itself: stage i + 1 at row i, stage N kept
            assert np.array_equal(rec["pred"][j, 0, :6], t["cand_X"][j, max(w, 0), 1:]) and np.array_equal(rec["pred"][j, 0, 6], t["cand_X"][j, max(w, 0), 6])
        for k in range(3):                              # member=k: always candidate k
            vk = visualisation_inputs(ms.multistart_record(res, g, member=k), 0)
            assert all(np.array_equal(vk["pred"][j + 1], t["cand_X"][j, k][:, :2]) for j in range(L))
            assert np.array_equal(vk["trajectory"], v["trajectory"])
    t = res["record"][1]
    assert t["winner"][1] == -1 and not t["u"][1].any()                                               # the case itself: a lost step
    assert np.array_equal(visualisation_inputs(ms.multistart_record(res, 1), 0)["pred"][2], t["cand_X"][1, 0][:, :2])


def test_multistart_record_refuses_clearly():
    from mpc_gpu import multistart as ms
    res = rc.synthetic_result()
    for g in (0, 1.0, True, "1", 4):
        with pytest.raises(ValueError, match="not recorded"):
            ms.multistart_record(res, g)
    with pytest.raises(ValueError, match="without a record"):
        ms.multistart_record({k: v for k, v in res.items() if k != "record"}, 1)
    for member in (3, -1, 1.0, True, "0"):
        with pytest.raises(ValueError, match="member"):
            ms.multistart_record(res, 1, member=member)
    noplans = rc.synthetic_result(plans=False)
    with pytest.raises(ValueError, match="record_plans=False"):
        ms.multistart_record(noplans, 3)
    with pytest.raises(ValueError, match="record_plans=False"):
        ms.multistart_record(noplans, 3, member=0)
