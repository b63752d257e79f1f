"""The interior point's PATH of every solve kernel against the oracle's: (mu, sigma, alpha, cmax) of every iteration (mpc_debug_trace) inside the band
of ip_trace_cases.py (rule, floors and margin from the reference alone; test_ip_trace_host.py proves them on the CPU).

Every other parity test judges a solve by where it ends, and the interior point is a contraction: a kernel whose centring target, step-to-boundary
fraction, complementarity mean or cold start is off in the sixth digit ends at the same point after the same number of iterations.  Its trace does not.

Fresh handles, a stream of the test's own.  The iterate every GPU solve starts from is read back and handed to the oracle, so one solve is compared,
never an accumulated difference.
  A  every level-0 name of kernel_configs.configs, explicit look-ahead (solve_dev) and device look-ahead (closed_loop_step_dev without step flags);
  B  the feature-level kernels of feature_kernel_cases, group by group (75 of the 78: ip_trace_cases.OPEN_KERNELS holds the three left out, the
     entry that left the band and the figures); one kernel per family again under an explicit slack schedule;
  C  where a row could land in the wrong place: packed mappings with a partly empty last wavefront, the smallest shapes of every mapping, a batch
     under instance scheduling, rows behind the iteration count, the block of an idle instance;
  D  the iteration cap; E the SQP loop; F tracing changes no result; G the arguments of mpc_debug_trace.
With IP_TRACE_RECORD=<file> in the environment the per-section, per-family figures are written there (profiles/ip_trace_parity.json)."""
import json
import os

import numpy as np
import pytest

import feature_kernel_cases as fk
import ip_trace_cases as it
import sqp_cases as sc
from feature_loop import mg, on_own_stream, smallest_scheduled_batch
from kernel_configs import apply, configs

pytestmark = pytest.mark.gpu
B = it.PLACEMENT_B
_RECORD = {}


def _family(name):
    return {"rti_solve_kernel": "one", "rti_split_kernel": "split", "rti_wide_kernel": "wide"}[name.split("<")[0]]


def _note(section, name, j):
    """one judged solve into the record: per section and kernel family the worst err / tol and the rows compared"""
    e = _RECORD.setdefault(section, {}).setdefault(_family(name), dict(kernels=[]))
    if name not in e["kernels"]:
        e["kernels"].append(name)
    kernels = e.pop("kernels")
    it.merge(e, j)
    e["kernels"] = kernels
    path = os.environ.get("IP_TRACE_RECORD")
    if path:
        with open(path, "w") as f:
            json.dump({s: {fam: dict(v, kernels=len(v["kernels"])) for fam, v in d.items()} for s, d in _RECORD.items()}, f, indent=1, sort_keys=True)


def _tensors(torch, **arrays):
    dev = torch.device("cuda:0")
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in arrays.items()}


def _traced(mpc_gpu, N, no, x0, goal, world, lookahead, setup=None, solves=2, ep_flags=None, scheduling=False, trace=True, **cfg_kw):
    """`solves` solves of one fresh handle from the cold guess, the record read after each.  world: the explicit look-ahead P
    (lookahead False: mpc_solve_dev) or the obstacle states (True: the fused entry without a step flag; with ep_flags: under STEP_METRICS alone, which moves nothing).  setup(s, keep): lane mapping and features;
    device arrays the handle reads in place go into `keep`.  Returns (kernel name, [dict(X0, U0, X, U, u0, cost, status, iters, trace, order)])"""
    import torch
    Bn = len(x0)
    c = lambda a: a.cpu().numpy().copy()
    q = torch.cuda.current_stream().cuda_stream
    out, keep = [], {}
    with mpc_gpu.BatchedMpc(N, no, 0.1 * N, max_batch=Bn, **cfg_kw) as s:
        s.set_instance_scheduling(bool(scheduling))
        if setup is not None:
            setup(s, keep)
        name = s.kernel_name(Bn, lookahead=lookahead)
        d = _tensors(torch, x0=x0, goal=goal, world=world)
        z = lambda *shape, dt=torch.float64: torch.zeros(*shape, dtype=dt, device=d["x0"].device)
        X, U, u0, cost = z(Bn, N + 1, 5), z(Bn, N, 2), z(Bn, 2), z(Bn)
        status, iters = z(Bn, dt=torch.int32), z(Bn, dt=torch.int32)
        # an episode word is read under STEP_METRICS alone (bit 0: the episode is over, the instance idles), which takes all three episode arrays
        ep = None if ep_flags is None else dict(_tensors(torch, fl=ep_flags.astype(np.int32), ns=np.zeros(Bn, np.int32)), mm=z(Bn) + float("inf"))
        torch.cuda.current_stream().synchronize()
        s.reset_guess_dev(Bn, d["x0"], X, U, stream=q)
        if trace:
            first = s.debug_trace(True, Bn)
            assert first.shape == (Bn, int(s.cfg.qp_iter_max), 4) and not first.any()      # zero from enabling on
        for _ in range(solves):
            torch.cuda.current_stream().synchronize()
            X0, U0 = c(X), c(U)
            if lookahead and ep is not None:
                ep["fl"].copy_(_tensors(torch, fl=ep_flags.astype(np.int32))["fl"])      # (the bookkeeping of the launch before may have ended an episode)
                torch.cuda.current_stream().synchronize()
                s.closed_loop_step_dev(Bn, d["x0"], d["world"], d["goal"], X, U, u0, cost, status, iters, flags=mpc_gpu._lib.STEP_METRICS,
                                       min_margin=ep["mm"], ep_flags=ep["fl"], ep_steps=ep["ns"], stream=q)
            elif lookahead:
                s.closed_loop_step_dev(Bn, d["x0"], d["world"], d["goal"], X, U, u0, cost, status, iters, flags=0, stream=q)
            else:
                s.solve_dev(Bn, d["x0"], d["world"], d["goal"], X, U, u0, cost, status, iters, stream=q)
            torch.cuda.current_stream().synchronize()      # the record is read behind the stream the solve ran on
            out.append(dict(X0=X0, U0=U0, X=c(X), U=c(U), u0=c(u0), cost=c(cost), status=c(status), iters=c(iters),
                            trace=s.debug_trace(True, Bn) if trace else None, order=s.instance_order(Bn) if scheduling else None))
    return name, out


def _placement(r, first_solve, idle=None):
    """what the record must look like whatever the numbers: rows in front of iters[b] written (mu > 0), on the first solve behind enabling every row
    at and behind iters[b] exactly zero, the block of an idle instance zero"""
    why = []
    tr, iters = r["trace"], r["iters"]
    for b in range(len(iters)):
        if idle is not None and idle[b]:
            if tr[b].any(): why.append(f"instance {b} idles and its block was written")
            continue
        n = int(iters[b])
        if not (0 <= n <= tr.shape[1]): why.append(f"instance {b}: {n} iterations"); continue
        if not (tr[b, :n, 0] > 0.0).all(): why.append(f"instance {b}: a row in front of its {n} iterations has no mu")
        if first_solve and tr[b, n:].any(): why.append(f"instance {b}: rows at or behind its {n} iterations were written {np.argwhere(tr[b, n:])[:2].tolist()}")
    return why


def _judge(orc, prob, r, idx=None):
    """the record of the instances idx (default all) of a launch against the band of `prob` (its rows in the order of idx), from the iterate the launch
    started from"""
    idx = np.arange(len(r["iters"])) if idx is None else idx
    p = dict(prob, X=r["X0"][idx], U=r["U0"][idx])
    j = it.judge_trace(r["trace"][idx], r["iters"][idx], it.band_of(orc, p))
    why = []
    if j["first"] is not None:
        b, k, col, g, o, tol = j["first"]
        why.append(f"{j['offending']} entries beyond the band, worst err / tol {j['worst']:.3g}; first: instance {int(idx[b])} iteration {k} {col} {g!r} vs {o!r} (tol {tol:.2e})")
    if j["short"]:
        why.append(f"iteration counts (instance, GPU, oracle): {[(int(idx[b]), g, o) for b, g, o in j['short']]}")
    if j["rows"] == 0:
        why.append("no row compared")
    return j, why


# ---------------------------------------------------------------------------------------------------------------- A: level-0 kernels
def _tags(name):
    fam, args = name.rstrip(">").split("<")
    a = args.split(", ")
    t = set()
    if fam == "rti_split_kernel":
        if a[2] == "true": t.add("W2")
        if a[4] == "true": t.add("block-2")
    if fam == "rti_solve_kernel":
        if a[2] == "0": t.add("systolic")
        if a[2] == "1": t.add("MFMA")
    return t


def _level0(mg, lookahead):
    mpc_gpu, orc = mg
    cfgs = configs(mpc_gpu, batch=B, lookahead=lookahead)
    bad, ran, refused, tags = [], [], [], set()
    for N, no, ov, name in cfgs:
        prob = it.cold(orc, N, no, B)
        try:
            got, rs = _traced(mpc_gpu, N, no, prob["x0"], prob["goal"], prob["obst"] if lookahead else prob["P"], lookahead, setup=lambda s, keep: apply(s, ov))
        except mpc_gpu.MpcError as e:
            assert "no kernel variant" in str(e), (name, str(e))      # a combination of overrides the dispatcher refuses at the launch (test_gpu_every_kernel.py)
            refused.append(name)
            continue
        assert got == name, (got, name)
        ran.append(got); tags |= _tags(got)
        for k, r in enumerate(rs):
            j, why = _judge(orc, prob, r)
            why += _placement(r, k == 0)
            _note("A-lookahead" if lookahead else "A-explicit", got, j)
            print(f"IP-TRACE A {got} N {N} n_obst {no} lookahead {lookahead} solve {k}: rows {j['rows']} of {j['oracle_rows']} worst {j['worst']:.3g} "
                  f"by column {[float(f'{v:.2g}') for v in j['worst_by_column']]} loose {j['loose']} {'FAILED: ' + '; '.join(why) if why else 'ok'}")
            if why:
                bad.append((got, k, why))
    print(f"IP-TRACE A lookahead {lookahead}: {len(set(ran))} kernel names ran, refused {refused}")
    assert not bad, bad
    assert len(set(ran)) >= 40 and {"W2", "block-2", "systolic", "MFMA"} <= tags, (sorted(set(ran)), tags, refused)


@pytest.mark.parametrize("lookahead", (False, True))
def test_every_level0_kernel_walks_the_oracles_path(mg, lookahead):
    on_own_stream(_level0, mg, lookahead)


# ---------------------------------------------------------------------------------------------------------------- B: feature kernels
def _feature_setup(mpc_gpu, case, inp, alpha=None):
    def setup(s, keep):
        import torch
        fk.configure(s, case)
        keep.update(_tensors(torch, yref=inp["yref"], offset=inp["offset"].astype(np.int32)))
        s.set_reference(keep["yref"], keep["offset"])
        if inp["level"] >= 2:
            keep.update(_tensors(torch, W=inp["W"], We=inp["We"], r_safe=inp["r_safe"]))
            s.set_instance_params(W=keep["W"], We=keep["We"], r_safe=keep["r_safe"])
        if inp["level"] >= 3:
            keep.update(_tensors(torch, words=mpc_gpu.pack_obstacle_mask(inp["mask"]).view(np.int32)))
            s.set_obstacle_mask(keep["words"])
        if inp["level"] >= 4:
            keep.update(_tensors(torch, table=mpc_gpu.pack_instance_bounds(s.cfg, len(inp["x0"]), **inp["bounds"])))
            s.set_instance_bounds_dev(keep["table"])
        if alpha is not None:
            keep.update(_tensors(torch, alpha=alpha))
            s.set_slack_schedule(keep["alpha"])
        torch.cuda.current_stream().synchronize()
    return setup


def _feature_case(mg, case, inp, alpha, section, bad):
    mpc_gpu, orc = mg
    name, rs = _traced(mpc_gpu, inp["N"], inp["no"], inp["x0"], inp["goal"], inp["obst"], True, setup=_feature_setup(mpc_gpu, case, inp, alpha),
                       ep_flags=inp["ep_flags"])
    assert name == case["name"], (name, case["name"])
    for k, r in enumerate(rs):
        total, why = {}, _placement(r, k == 0, idle=inp["ep_flags"] != 0)
        if k == 1 and alpha is None and (inp["N"], inp["no"], inp["level"]) in it.UNJUDGED_SECOND:
            assert not why, (name, why)
            continue
        for idx, prob in it.feature_groups(orc, inp, alpha=alpha, X=r["X0"], U=r["U0"]):
            j, w = _judge(orc, prob, r, idx)
            it.merge(total, j); why += w
            _note(section, name, j)
        print(f"IP-TRACE {section} {name} N {inp['N']} n_obst {inp['no']} solve {k}: rows {total['rows']} of {total['oracle_rows']} worst {total['worst']:.3g} "
              f"loose {total['loose']} {'FAILED: ' + '; '.join(why) if why else 'ok'}")
        if why:
            bad.append((name, k, why))
    return name


def _features(mg, family, level):
    bad, ran = [], []
    cases = [c for c in fk.cases_of(family, level) if c["name"] not in it.OPEN_KERNELS]
    for case in cases:
        ran.append(_feature_case(mg, case, fk.inputs(mg[1], case), None, "B", bad))
    print(f"IP-TRACE B {family} level {level}: {len(set(ran))} kernel names ran")
    assert not bad, bad
    assert sorted(ran) == sorted(c["name"] for c in cases), ran


@pytest.mark.parametrize("level", fk.LEVELS)
@pytest.mark.parametrize("family", fk.FAMILIES)
def test_every_feature_kernel_walks_the_oracles_path(mg, family, level):
    on_own_stream(_features, mg, family, level)


def test_the_feature_parametrisation_covers_the_78_kernels_but_the_open_ones():
    names = {c["name"] for f in fk.FAMILIES for l in fk.LEVELS for c in fk.cases_of(f, l)}
    assert len(names) == 78 == len(fk.enumerate_cases()) and set(it.OPEN_KERNELS) <= names
    assert len(names - set(it.OPEN_KERNELS)) == 75            # ip_trace_cases.OPEN_KERNELS: one entry of one problem, the side at fault undecided


def _scheduled_features(mg, family):
    import slack_schedule_cases as ss
    bad = []
    case = it.schedule_case(family)
    prob = ss.feature_problem(mg[1], case, "crowded")
    _feature_case(mg, case, prob["inp"], prob["alpha"], "B-slack-schedule", bad)
    assert not bad, bad


@pytest.mark.parametrize("family", fk.FAMILIES)
def test_a_feature_kernel_under_an_explicit_slack_schedule_walks_the_oracles_path(mg, family):
    on_own_stream(_scheduled_features, mg, family)


# ---------------------------------------------------------------------------------------------------------------- C: where a row could land
def _mapping(mg, mapping, N, no):
    mpc_gpu, orc = mg
    lps = {"lps3": 3, "lps2": 2, "one": 1}.get(mapping)
    prob = it.cold(orc, N, no, B)
    name, rs = _traced(mpc_gpu, N, no, prob["x0"], prob["goal"], prob["P"], False, setup=None if lps is None else (lambda s, keep: s.set_lanes_per_stage(lps)))
    want = {"lps3": "rti_split_kernel<", "lps2": "rti_split_kernel<", "one": "rti_solve_kernel<", "wide": "rti_wide_kernel<"}.get(mapping, "rti_")
    assert name.startswith(want) and (lps in (None, 1) or name.split(", ")[1] == str(lps)), name
    bad = []
    for k, r in enumerate(rs):
        j, why = _judge(orc, prob, r)
        why += _placement(r, k == 0)
        _note("C-mappings", name, j)
        print(f"IP-TRACE C {mapping} {name} N {N} n_obst {no} solve {k}: rows {j['rows']} of {j['oracle_rows']} worst {j['worst']:.3g} {'FAILED: ' + '; '.join(why) if why else 'ok'}")
        if why:
            bad.append((name, k, why))
    assert not bad, bad


@pytest.mark.parametrize("mapping,N,no", [(m, N, no) for m, shapes in it.MAPPING_SHAPES.items() for N, no in shapes])
def test_the_smallest_shapes_of_every_mapping(mg, mapping, N, no):
    on_own_stream(_mapping, mg, mapping, N, no)


def _packed(mg, lanes, N, no):
    mpc_gpu, orc = mg
    Bp = it.PACKED_B
    assert (Bp * lanes) % 64 != 0 and Bp * lanes > 64      # more than one wavefront, the last partly empty
    prob = it.cold(orc, N, no, Bp)
    name, rs = _traced(mpc_gpu, N, no, prob["x0"], prob["goal"], prob["P"], False, setup=lambda s, keep: (s.set_lanes_per_stage(1), s.set_lanes_per_instance(lanes)))
    assert name.startswith(f"rti_solve_kernel<{no}, {lanes},"), name
    bad = []
    for k, r in enumerate(rs):
        j, why = _judge(orc, prob, r)
        why += _placement(r, k == 0)
        _note("C-packed", name, j)
        print(f"IP-TRACE C packed {name} N {N} n_obst {no} solve {k}: rows {j['rows']} of {j['oracle_rows']} worst {j['worst']:.3g} {'FAILED: ' + '; '.join(why) if why else 'ok'}")
        if why:
            bad.append((name, k, why))
    assert not bad, bad


@pytest.mark.parametrize("lanes,N,no", it.PACKED)
def test_packed_mappings_with_a_partly_empty_last_wavefront(mg, lanes, N, no):
    on_own_stream(_packed, mg, lanes, N, no)


def _under_scheduling(mg):
    mpc_gpu, orc = mg
    N, no = it.SCHEDULED_SHAPE
    Bs = smallest_scheduled_batch(mpc_gpu, N, no)
    assert Bs >= it.SCHEDULED_JUDGED
    prob = it.scheduled_problem(orc, Bs)
    name, rs = _traced(mpc_gpu, N, no, prob["x0"], prob["goal"], prob["P"], False, solves=3, scheduling=True)
    # the permutation in effect for a launch is the one reported behind the launch before it
    order = rs[0]["order"]
    assert order is not None and sorted(order.tolist()) == list(range(Bs)) and not np.array_equal(order, np.arange(Bs)), order
    assert not np.array_equal(order[:it.SCHEDULED_JUDGED], np.arange(it.SCHEDULED_JUDGED))
    idx = np.arange(it.SCHEDULED_JUDGED)
    sub = {k: (v[idx] if isinstance(v, np.ndarray) else v) for k, v in prob.items()}
    bad = []
    for k, r in enumerate(rs):
        j, why = _judge(orc, sub, r, idx)
        why += _placement(r, k == 0)
        _note("C-scheduled", name, j)
        print(f"IP-TRACE C scheduled {name} batch {Bs} solve {k}: rows {j['rows']} of {j['oracle_rows']} worst {j['worst']:.3g} {'FAILED: ' + '; '.join(why[:6]) if why else 'ok'}")
        if why:
            bad.append((name, k, why[:6]))
    assert not bad, bad


def test_row_block_b_is_instance_b_under_instance_scheduling(mg):
    on_own_stream(_under_scheduling, mg)


# ---------------------------------------------------------------------------------------------------------------- D: the cap
def _cap(mg):
    mpc_gpu, orc = mg
    N, no = it.CAP_SHAPE
    prob = it.cold(orc, N, no, B, qp_iter_max=it.CAP_ITER_MAX)
    name, (r,) = _traced(mpc_gpu, N, no, prob["x0"], prob["goal"], prob["P"], False, solves=1, qp_iter_max=it.CAP_ITER_MAX)
    assert r["trace"].shape == (B, it.CAP_ITER_MAX, 4)
    assert (r["iters"] == it.CAP_ITER_MAX).all(), r["iters"]                     # every instance ends at the cap
    j, why = _judge(orc, prob, r)
    why += _placement(r, True)
    assert j["rows"] == B * it.CAP_ITER_MAX, j                                   # rows 0 .. 4 of every instance
    # row 0 of instance b + 1 is its own (a write at row iter_max of instance b would land there): judged above, and the mu of a cold start is the same
    # constant in every instance only by the oracle's say
    _note("D", name, j)
    print(f"IP-TRACE D {name}: rows {j['rows']} worst {j['worst']:.3g} {'FAILED: ' + '; '.join(why) if why else 'ok'}")
    assert not why, why


def test_at_the_iteration_cap_every_row_is_its_instances_own(mg):
    on_own_stream(_cap, mg)


# ---------------------------------------------------------------------------------------------------------------- E: SQP
def _sqp(mg, cid):
    mpc_gpu, orc = mg
    c = sc.case(cid)
    inp = sc.inputs(orc, c)
    N, no = inp["N"], inp["no"]
    fin = sc.finite_instances()
    rows = lambda idx: it.problem(inp["cfg"], inp["x0"][idx], inp["P"][idx], inp["goal"][idx], inp["X0"][idx], inp["U0"][idx])
    setup = lambda tol: (lambda s, keep: (s.set_lanes_per_stage(c["lps"]) if c["family"] != "wide" else None, s.set_sqp(2, tol)))
    # one iteration of the level-5 kernel (step_tol +inf stops behind the first): its record and its iteration counts
    name, (one,) = _traced(mpc_gpu, N, no, inp["x0"], inp["goal"], inp["P"], False, setup=setup(float("inf")), solves=1)
    assert name == c["name"], (name, c["name"])
    j1, why = _judge(orc, rows(fin), one, fin)
    why += _placement(one, True)
    assert not one["trace"][sc.NAN_INSTANCE].any()               # (a NaN in x0: refused in front of the interior point)
    # two iterations in one launch: the record is the second's, which started from the first's result -- the single launch's, bit for bit
    name2, (two,) = _traced(mpc_gpu, N, no, inp["x0"], inp["goal"], inp["P"], False, setup=setup(0.0), solves=1)
    assert name2 == name
    ok = fin[one["status"][fin] != 4]
    second = dict(two, X0=one["X"], U0=one["U"], iters=two["iters"] - one["iters"])
    j2, w2 = _judge(orc, rows(ok), second, ok)
    why += w2
    for b in ok:      # rows behind the second iteration's own are the first's, left in place, or zero
        n2, n1 = int(second["iters"][b]), int(one["iters"][b])
        if not (np.array_equal(two["trace"][b, n2:n1], one["trace"][b, n2:n1]) and not two["trace"][b, max(n1, n2):].any()):
            why.append(f"instance {b}: rows behind the second iteration's {n2} are neither the first's nor zero")
    _note("E-first", name, j1); _note("E-second", name, j2)
    print(f"IP-TRACE E {name}: first iteration rows {j1['rows']} worst {j1['worst']:.3g}; second rows {j2['rows']} worst {j2['worst']:.3g} "
          f"{'FAILED: ' + '; '.join(why) if why else 'ok'}")
    assert not why, why
    assert j2["rows"] > 0


@pytest.mark.parametrize("cid", it.SQP_CASES)
def test_the_sqp_loops_record_is_its_last_iterations(mg, cid):
    on_own_stream(_sqp, mg, cid)


# ---------------------------------------------------------------------------------------------------------------- F: tracing changes nothing
def _changes_nothing(mg, family):
    mpc_gpu, orc = mg
    N, no = it.FAMILY_SHAPES[family]
    prob = it.cold(orc, N, no, B)
    name, traced = _traced(mpc_gpu, N, no, prob["x0"], prob["goal"], prob["obst"], True)
    plain_name, plain = _traced(mpc_gpu, N, no, prob["x0"], prob["goal"], prob["obst"], True, trace=False)
    assert name == plain_name and _family(name) == family, (name, plain_name)
    for a, b in zip(traced, plain):
        for k in ("X", "U", "u0", "cost", "status", "iters"):
            assert np.array_equal(a[k], b[k]), (name, k)
    assert all(r["trace"].any() for r in traced)
    with mpc_gpu.BatchedMpc(N, no, 0.1 * N, max_batch=B) as s:
        s.debug_trace(True)
        s.reset_guess(prob["x0"])
        s.solve(prob["x0"], prob["obst"], prob["goal"])          # (the host entry: on the handle's own stream, which debug_trace waits for)
        assert s.debug_trace(True, B).any()
        held = s.debug_trace(False, B)
        assert held.any()                                        # switching off hands over what it held ...
        assert not s.debug_trace(False, B).any()
        assert not s.debug_trace(True, B).any()                  # ... and enabling again starts from zero


@pytest.mark.parametrize("family", fk.FAMILIES)
def test_tracing_changes_no_result(mg, family):
    on_own_stream(_changes_nothing, mg, family)


# ---------------------------------------------------------------------------------------------------------------- G: arguments
def test_debug_trace_refuses_a_batch_outside_the_handle(mg):
    mpc_gpu, _ = mg
    with mpc_gpu.BatchedMpc(20, 3, 2.0, max_batch=5) as s:
        for on in (True, False, True):
            for batch in (0, -1, 6, 2 ** 31 - 1):
                with pytest.raises(mpc_gpu.MpcError, match="batch"):
                    s.debug_trace(on, batch)
        assert s.debug_trace(True, 5).shape == (5, int(s.cfg.qp_iter_max), 4)
        assert s.debug_trace(True, 1).shape == (1, int(s.cfg.qp_iter_max), 4)
        assert s.debug_trace(True).shape[0] == 5
