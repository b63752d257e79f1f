"""What a seed sweep with on-device refill (run_seed_sweep) gives over the batch harness, and what the refill costs per control step, on the GPU.

Workload: the reference's experiment (RANDOM, N 20, 5 obstacles, Tf 2, QP_ITER 100, max_iter 400) over --seeds seeds (default 16384), in four forms:
  "chunks":     run_episodes on chunks of --slots episodes (default 1024), one after the other: what a caller did before;
  "one_batch":  run_episodes on ONE batch of all seeds with its default compaction;
  "sweep":      run_seed_sweep through --slots slots;
  "sweep_wide": run_seed_sweep through 4 x --slots slots.
Every form runs --reps times (default 3) behind one warm-up, the forms alternating rep by rep; wall time between device synchronises (scripts/measure.py's
alternate and wall).
Recorded per form: the times, their spread (max - min over median), episodes/s, fused steps launched.  Beside them the PREDICTED ratio of fused steps
sweep / chunks -- refill_schedule over the lengths of the chunks' own tables against the sum of the chunks' longest episodes -- and whether the sweep's
steps_run is what refill_schedule says (exactly, in one more run with poll_every = 1).

Per-step overhead (measure.per_call: HIP events on the step's stream, median of --launches single calls at --slots slots): mpc_episode_refill_dev with no slot finished,
with one slot refilled and with every slot refilled, each with and without the noise draw; mpc_noise_draw_dev alone; the fused step.

    python scripts/sweep_rate.py [--seeds 16384] [--slots 1024] [--reps 3] [--launches 30] [--out profiles/sweep_rates.json]
    python scripts/sweep_rate.py --trace off all all-nopred [--baseline-root DIR] [--trace-out profiles/sweep_trace_rates.json]

--ring-forms measures the per-seed features instead and writes profiles/sweep_ring_rates.json (profiles/sweep_rates.json is left alone): at every slot count
of --slot-counts (default 1024,4096) the forms
  "baseline":   run_seed_sweep of ANOTHER CHECKOUT (--baseline-root DIR, built there; its package and library are loaded beside this one, so the forms
                alternate in one process) -- the parent commit's sweep; left out without the option;
  "off":        run_seed_sweep with everything off: must equal "baseline" within the spread;
  "ring":       ring on, capacity = slots, ring_every = 25;
  "features":   per-seed radii + mask + bounds;
  "all":        every per-seed table, the status log and the ring;
the same protocol (a warm-up, then --reps runs per form, the forms alternating), and the per-call table for the refill with ONE slot refilled, ring on
against ring off, the ring fill and the status log kernel.

--trace FORM [FORM ...] (off, all, all-nopred) measures the per-seed trajectories instead and writes profiles/sweep_trace_rates.json: run_seed_sweep at --slots
slots over --seeds seeds with trace off, with every seed traced, and with every seed traced without the predicted horizons -- beside "baseline", the parent
commit's sweep, when --baseline-root is given.  The same protocol (a warm-up, then --reps runs per form, the forms alternating in one process); wall time
around the whole call, read-back of the rows to the host included, and solves/s = the table's solves over the median time.  Beside the forms: the trace
launches per call (HIP events, START and STEP, with and without pred) at --slots slots.
"""
import argparse
import json
import os
import sys

import numpy as np

import measure


def load_baseline(root):
    """the mpc_gpu package of another checkout under its own module name: its own Python, its own libmpcgpu.so (built there beforehand)"""
    import importlib.util
    pkg = os.path.join(root, "dynamic-obstacle-avoidance-mpc_amd", "mpc_gpu")
    spec = importlib.util.spec_from_file_location("mpc_gpu_baseline", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mpc_gpu_baseline"] = mod
    spec.loader.exec_module(mod)
    if not os.path.exists(mod._lib.LIB_PATH):
        raise SystemExit(f"{mod._lib.LIB_PATH} is missing: build the baseline checkout first")
    return mod


def ring_forms(a):
    torch = measure.require_gpu()
    import mpc_gpu
    import sweep_cases as sc
    import sweep_feature_cases as fc
    L = mpc_gpu._lib
    E, scen = a.seeds, a.scenario
    prob = dict(sc.PROBLEM, max_iter=400)
    base = load_baseline(a.baseline_root) if a.baseline_root else None
    feat = fc.feature_kwargs("all", E)
    some = {n: feat[n] for n in ("r_safe", "r_hit", "active", "bounds")}
    out = dict(workload=dict(scenario=scen, seeds=E, reps=a.reps, ring_every=25, **prob), by_slots={})
    for S in [int(x) for x in a.slot_counts.split(",")]:
        forms = {}
        if base is not None:
            forms["baseline"] = lambda: base.run_seed_sweep(sc.START, sc.GOAL, scen, (0, E), S, **prob)
        forms["off"] = lambda: mpc_gpu.run_seed_sweep(sc.START, sc.GOAL, scen, (0, E), S, **prob)
        forms["ring"] = lambda: mpc_gpu.run_seed_sweep(sc.START, sc.GOAL, scen, (0, E), S, ring=S, ring_every=25, **prob)
        forms["features"] = lambda: mpc_gpu.run_seed_sweep(sc.START, sc.GOAL, scen, (0, E), S, **some, **prob)
        forms["all"] = lambda: mpc_gpu.run_seed_sweep(sc.START, sc.GOAL, scen, (0, E), S, ring=S, ring_every=25, status_log=True, **feat, **prob)
        runs = measure.alternate({f: (lambda fn=fn: measure.wall(fn, torch)) for f, fn in forms.items()}, a.reps, on_run=lambda rep, f, v: print(json.dumps(
            dict(slots=S, rep=rep, form=f, seconds=v[0], steps_run=v[1]["steps_run"])), flush=True))
        res, last = {}, {f: r[-1][1] for f, r in runs.items()}
        for f in forms:
            ts = [sec for sec, _ in runs[f]]
            med, spread = measure.summary(ts)
            res[f] = dict(seconds=ts, median_s=med, spread=spread, episodes_per_s=float(E / med), fused_steps=int(last[f]["steps_run"]),
                          ms_per_step=float(1e3 * med / last[f]["steps_run"]))
        spread = max(r["spread"] for r in res.values())
        summary = dict(largest_spread=spread, ring_over_off=res["ring"]["median_s"] / res["off"]["median_s"],
                       ring_faster_than_off_beyond_spread=bool(res["ring"]["median_s"] < res["off"]["median_s"] * (1 - spread)),
                       features_over_off=res["features"]["median_s"] / res["off"]["median_s"], all_over_off=res["all"]["median_s"] / res["off"]["median_s"],
                       ring_rows_equal_off=bool(np.array_equal(last["ring"]["table"], last["off"]["table"])))
        if base is not None:
            summary.update(off_over_baseline=res["off"]["median_s"] / res["baseline"]["median_s"],
                           off_equals_baseline_within_spread=bool(abs(res["off"]["median_s"] / res["baseline"]["median_s"] - 1) <= spread),
                           off_rows_equal_baseline=bool(np.array_equal(last["off"]["table"], last["baseline"]["table"])))
        out["by_slots"][str(S)] = dict(forms=res, summary=summary)
        print(json.dumps({str(S): out["by_slots"][str(S)]}), flush=True)

    # ---- the per-call table: ONE slot refilled, ring on against ring off; the ring fill; the status log
    S = int(a.slot_counts.split(",")[0])
    dev = torch.device("cuda", 0)
    over = {}
    with mpc_gpu.BatchedMpc(max_batch=S, **sc.PROBLEM) as m, measure.own_stream(torch) as st:
        cs = st.cuda_stream
        plain = sc.Plain(torch, dev)
        arr = sc.SlotArrays(plain, m, S, E, L.lib().mpc_noise_state_words())
        words = L.lib().mpc_noise_state_words()
        ring_state, ring_obst = plain.i32(S, words), plain.f64(S, m.n_obst, 4)
        ring_tag, seed_src, log = plain.i32(S, init=-1), plain.i32(E, init=-1), plain.i32(S, 4)
        step_flags = L.STEP_SHIFT | L.STEP_PLANT | L.STEP_OBSTACLES | L.STEP_METRICS | L.STEP_RESET_ON_FAIL | L.STEP_ALIAS_BUG
        fl = L.REFILL_ALIAS_BUG | L.REFILL_DRAW_NOISE

        timed = lambda fn, before=None: measure.per_call(torch, st, fn, a.launches, before)

        for _ in range(10):                     # a few control steps in: every slot runs
            arr.refill(m, scen, 0, 400, fl, cs); arr.step(m, step_flags, cs)
        st.synchronize()
        assert int((arr.flags & 1).sum().item()) == 0
        one = lambda: arr.flags[S // 2:S // 2 + 1].fill_(1)
        over["refill_one_slot_ring_off"] = timed(lambda: arr.refill(m, scen, 0, 400, fl, cs), before=one)
        over["refill_nothing_finished_ring_off"] = timed(lambda: arr.refill(m, scen, 0, 400, fl, cs))
        m.episode_ring_dev(S, ring_state, ring_obst, ring_tag, seed_src)
        over["ring_fill_every_entry"] = timed(lambda: m.episode_ring_fill_dev(scen, 0, E, arr.cursor, stream=cs), before=lambda: ring_tag.fill_(-1))
        over["ring_fill_nothing_to_seed"] = timed(lambda: m.episode_ring_fill_dev(scen, 0, E, arr.cursor, stream=cs))
        over["refill_one_slot_ring_on"] = timed(lambda: arr.refill(m, scen, 0, 400, fl, cs), before=one)
        st.synchronize()
        over["refill_one_slot_ring_on_hits"] = int((seed_src == 1).sum().item())          # (every timed refill found its index in the ring)
        over["refill_one_slot_ring_on_misses"] = int((seed_src == 0).sum().item())
        over["refill_nothing_finished_ring_on"] = timed(lambda: arr.refill(m, scen, 0, 400, fl, cs))
        over["status_log"] = timed(lambda: m.episode_status_log_dev(S, arr.status, arr.flags, arr.steps, log, stream=cs))
        m.episode_ring_dev(0)
    out["per_call"] = dict(slots=S, launches=a.launches, **over)
    print(json.dumps(dict(per_call=out["per_call"])), flush=True)
    measure.write_json(a.ring_out, out)


def trace_forms(a):
    torch = measure.require_gpu()
    import mpc_gpu
    import sweep_cases as sc
    L = mpc_gpu._lib
    E, S, scen = a.seeds, a.slots, a.scenario
    prob = dict(sc.PROBLEM, max_iter=400)
    base = load_baseline(a.baseline_root) if a.baseline_root else None
    run = lambda **kw: mpc_gpu.run_seed_sweep(sc.START, sc.GOAL, scen, (0, E), S, trace_max_bytes=2 ** 40, **kw, **prob)
    forms = {}
    if base is not None:
        forms["baseline"] = lambda: base.run_seed_sweep(sc.START, sc.GOAL, scen, (0, E), S, **prob)
    for f in a.trace:
        forms[f] = {"off": lambda: run(), "all": lambda: run(trace=True), "all-nopred": lambda: run(trace=True, trace_pred=False)}[f]
    last = {}

    def timed_form(f, fn):      # seconds; of the result only what the record needs is kept (a trace of every seed is gigabytes on the host: one at a time)
        dt, r = measure.wall(fn, torch)
        last[f] = dict(table=r["table"], steps_run=r["steps_run"], solves=r["solves"], traced=len(r.get("trace", ())),
                       trace_rows=int(sum(t["u"].shape[0] for t in r["trace"].values())) if "trace" in r else 0)
        return dt

    times = measure.alternate({f: (lambda f=f, fn=fn: timed_form(f, fn)) for f, fn in forms.items()}, a.reps, on_run=lambda rep, f, dt: print(json.dumps(
        dict(slots=S, rep=rep, form=f, seconds=dt, steps_run=last[f]["steps_run"])), flush=True))
    res = {}
    for f in forms:
        med, spread = measure.summary(times[f])
        res[f] = dict(seconds=times[f], median_s=med, spread=spread, solves=int(last[f]["solves"]), solves_per_s=float(last[f]["solves"] / med),
                      episodes_per_s=float(E / med), fused_steps=int(last[f]["steps_run"]), ms_per_step=float(1e3 * med / last[f]["steps_run"]),
                      traced_seeds=int(last[f]["traced"]), traced_steps=int(last[f]["trace_rows"]))
    ref = "off" if "off" in res else next(iter(res))
    summary = dict(largest_spread=max(r["spread"] for r in res.values()))
    for f in res:
        if f != ref:
            summary[f.replace("-", "_") + "_over_" + ref] = res[f]["median_s"] / res[ref]["median_s"]
            summary[f.replace("-", "_") + "_rows_equal_" + ref] = bool(np.array_equal(last[f]["table"], last[ref]["table"]))
    if base is not None and "off" in res:
        spread = max(res["off"]["spread"], res["baseline"]["spread"])
        summary.update(off_over_baseline=res["off"]["median_s"] / res["baseline"]["median_s"], off_baseline_spread=spread,
                       off_equals_baseline_within_spread=bool(abs(res["off"]["median_s"] / res["baseline"]["median_s"] - 1) <= spread))
    for f, pred in (("all", True), ("all-nopred", False)):
        if f in res:
            res[f]["device_bytes"] = int(mpc_gpu.trace_bytes(E, 400, sc.PROBLEM["N"], sc.PROBLEM["n_obst"], pred=pred))
    out = dict(workload=dict(scenario=scen, seeds=E, slots=S, reps=a.reps, **prob), forms=res, summary=summary)
    print(json.dumps(out), flush=True)

    # ---- the trace launches on their own: every slot a few steps into a traced episode
    dev = torch.device("cuda", 0)
    over = {}
    with mpc_gpu.BatchedMpc(max_batch=S, **sc.PROBLEM) as m, measure.own_stream(torch) as st:
        cs = st.cuda_stream
        plain = sc.Plain(torch, dev)
        arr = sc.SlotArrays(plain, m, S, E, L.lib().mpc_noise_state_words())
        N, no, T = m.N, m.n_obst, 400
        step_flags = L.STEP_SHIFT | L.STEP_PLANT | L.STEP_OBSTACLES | L.STEP_METRICS | L.STEP_RESET_ON_FAIL | L.STEP_ALIAS_BUG
        fl = L.REFILL_ALIAS_BUG | L.REFILL_DRAW_NOISE
        u0 = plain.f64(S, 2)
        seed_row = plain.i32(E, init=-1); seed_row[:S] = torch.arange(S, dtype=torch.int32, device=dev)
        t = dict(seed_row=seed_row, slot_state=plain.i32(S, 2), len=plain.i32(S), x=plain.f64(S, T + 1, 5), obst=plain.f64(S, T + 1, no, 4), u=plain.f64(S, T, 2),
                 status=plain.i32(S, T), iters=plain.i32(S, T), pred=plain.f64(S, T, N + 1, 5))

        timed = lambda fn, before=None: measure.per_call(torch, st, fn, a.launches, before)

        def step():
            m.closed_loop_step_dev(S, arr.x0, arr.obst, arr.goal, arr.X, arr.U, u0, None, arr.status, arr.iters, arr.noise, flags=step_flags, min_margin=arr.margin,
                                   ep_flags=arr.flags, ep_steps=arr.steps, stream=cs)
        start = lambda: m.episode_trace_dev(S, L.TRACE_START, arr.slot_seed, arr.x0, arr.obst, ep_flags=arr.flags, ep_steps=arr.steps, stream=cs)
        record = lambda: m.episode_trace_dev(S, L.TRACE_STEP, arr.slot_seed, arr.x0, arr.obst, arr.X, u0, arr.status, arr.iters, arr.flags, arr.steps, stream=cs)
        for tag, pred in (("", t["pred"]), ("_nopred", None)):
            t["slot_state"].copy_(torch.tensor([-1, 0], dtype=torch.int32, device=dev).repeat(S, 1))
            arr.flags.fill_(1); arr.steps.zero_(); arr.slot_seed.fill_(-1); arr.cursor.zero_()
            m.episode_trace_set_dev(S, T, **dict(t, pred=pred))
            arr.refill(m, scen, 0, 400, fl, cs)
            over["trace_start_every_slot_starts" + tag] = timed(start, before=lambda: t["slot_state"][:, 0].fill_(-1))
            over["trace_start_nothing_starts" + tag] = timed(start)
            over["trace_step_every_slot_stepped" + tag] = timed(record, before=lambda: (arr.refill(m, scen, 0, 400, fl, cs), step()))
            over["trace_step_nothing_stepped" + tag] = timed(record)
            st.synchronize()
            over["rows_with_every_timed_step_recorded" + tag] = int((t["len"] == a.launches).sum().item())      # (of --slots; an episode shorter than that has ended)
        m.episode_trace_set_dev(0)
    out["per_call"] = dict(slots=S, launches=a.launches, **over)
    print(json.dumps(dict(per_call=out["per_call"])), flush=True)
    measure.write_json(a.trace_out, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", nargs="+", choices=["off", "all", "all-nopred"], default=None)
    ap.add_argument("--trace-out", default=os.path.join(measure.ROOT, "profiles", "sweep_trace_rates.json"))
    ap.add_argument("--ring-forms", action="store_true")
    ap.add_argument("--slot-counts", default="1024,4096")
    ap.add_argument("--baseline-root", default=None)
    ap.add_argument("--ring-out", default=os.path.join(measure.ROOT, "profiles", "sweep_ring_rates.json"))
    ap.add_argument("--seeds", type=int, default=16384)
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--scenario", default="RANDOM")
    ap.add_argument("--out", default=os.path.join(measure.ROOT, "profiles", "sweep_rates.json"))
    a = ap.parse_args()
    if a.ring_forms:
        return ring_forms(a)
    if a.trace:
        return trace_forms(a)
    torch = measure.require_gpu()
    import mpc_gpu
    import sweep_cases as sc
    L = mpc_gpu._lib
    E, S, scen = a.seeds, a.slots, a.scenario
    prob = dict(sc.PROBLEM, max_iter=400)
    x0 = lambda n: np.tile(sc.START, (n, 1))
    goal = lambda n: np.tile(sc.GOAL, (n, 1))

    def chunks():
        tabs, steps = [], 0
        for c0 in range(0, E, S):
            n = min(S, E - c0)
            r = mpc_gpu.run_episodes(x0(n), goal(n), scen, first_seed=c0, **prob)
            tabs.append(r["table"]); steps += r["steps_run"]
        return dict(table=np.concatenate(tabs), steps_run=steps)

    forms = {"chunks": chunks,
             "one_batch": lambda: mpc_gpu.run_episodes(x0(E), goal(E), scen, first_seed=0, **prob),
             "sweep": lambda: mpc_gpu.run_seed_sweep(sc.START, sc.GOAL, scen, (0, E), S, **prob),
             "sweep_wide": lambda: mpc_gpu.run_seed_sweep(sc.START, sc.GOAL, scen, (0, E), 4 * S, **prob)}
    runs = measure.alternate({f: (lambda fn=fn: measure.wall(fn, torch)) for f, fn in forms.items()}, a.reps, on_run=lambda rep, f, v: print(json.dumps(
        dict(rep=rep, form=f, seconds=v[0], steps_run=v[1]["steps_run"])), flush=True))
    res, last = {}, {f: r[-1][1] for f, r in runs.items()}
    for f in forms:
        ts = [sec for sec, _ in runs[f]]
        med, spread = measure.summary(ts)
        res[f] = dict(seconds=ts, median_s=med, spread=spread, episodes_per_s=float(E / med), fused_steps=int(last[f]["steps_run"]),
                      reached=float(last[f]["table"][:, 1].mean()), mean_steps=float(last[f]["table"][:, 4].mean()))
    base = last["chunks"]["table"]
    lengths = (base[:, 4] + base[:, 1]).astype(int)
    chunk_steps = int(sum(lengths[c0:c0 + S].max() for c0 in range(0, E, S)))
    pred = {}
    for f, slots in (("sweep", S), ("sweep_wide", 4 * S)):
        T = mpc_gpu.refill_schedule(lengths, slots)["steps"]
        launched = (-(-T // 25) + 1) * 25
        pred[f] = dict(slots=slots, schedule_steps=int(T), launched_steps_expected=int(launched), launched_steps=res[f]["fused_steps"],
                       steps_as_predicted=bool(res[f]["fused_steps"] == launched),
                       rows_equal_chunks=bool(np.array_equal(last[f]["table"], base)), rows_equal_fraction=float((last[f]["table"] == base).all(axis=1).mean()))
    exact = mpc_gpu.run_seed_sweep(sc.START, sc.GOAL, scen, (0, E), S, poll_every=1, **prob)
    pred["sweep"]["poll_every_1_steps"] = int(exact["steps_run"])
    pred["sweep"]["poll_every_1_steps_equal_schedule"] = bool(exact["steps_run"] == pred["sweep"]["schedule_steps"])
    sched = mpc_gpu.refill_schedule(lengths, S)
    pred["sweep"]["poll_every_1_schedule_equal_model"] = bool(np.array_equal(exact["schedule"][:, 0], sched["slot"]) and np.array_equal(exact["schedule"][:, 1], sched["start"]))
    summary = dict(chunk_fused_steps_from_lengths=chunk_steps, chunk_fused_steps_launched=res["chunks"]["fused_steps"],
                   predicted_step_ratio_sweep_over_chunks=pred["sweep"]["schedule_steps"] / chunk_steps,
                   measured_time_ratio_sweep_over_chunks=res["sweep"]["median_s"] / res["chunks"]["median_s"],
                   sweep_not_slower_than_chunks_beyond_spread=bool(res["sweep"]["median_s"] <= res["chunks"]["median_s"] * (1 + max(res["sweep"]["spread"], res["chunks"]["spread"]))),
                   one_batch_rows_equal_fraction=float((last["one_batch"]["table"] == base).all(axis=1).mean()))
    print(json.dumps(dict(forms=res, prediction=pred, summary=summary)), flush=True)

    # ---- the per-step overhead: single launches between HIP events
    dev = torch.device("cuda", 0)
    over = {}
    with mpc_gpu.BatchedMpc(max_batch=S, **sc.PROBLEM) as m, measure.own_stream(torch) as st:
        cs = st.cuda_stream
        arr = sc.SlotArrays(sc.Plain(torch, dev), m, S, E, L.lib().mpc_noise_state_words())
        step_flags = L.STEP_SHIFT | L.STEP_PLANT | L.STEP_OBSTACLES | L.STEP_METRICS | L.STEP_RESET_ON_FAIL | L.STEP_ALIAS_BUG
        base_fl = L.REFILL_ALIAS_BUG

        timed = lambda fn, before=None: measure.per_call(torch, st, fn, a.launches, before)

        def fresh():
            arr.flags.fill_(1); arr.slot_seed.fill_(-1); arr.cursor.zero_()

        for tag, fl in (("", base_fl), ("_with_noise", base_fl | L.REFILL_DRAW_NOISE)):
            over["refill_every_slot" + tag] = timed(lambda: arr.refill(m, scen, 0, 400, fl, cs), before=fresh)
        for _ in range(10):                     # a few control steps in: every slot runs
            arr.refill(m, scen, 0, 400, base_fl | L.REFILL_DRAW_NOISE, cs); arr.step(m, step_flags, cs)
        st.synchronize()
        assert int((arr.flags & 1).sum().item()) == 0
        for tag, fl in (("", base_fl), ("_with_noise", base_fl | L.REFILL_DRAW_NOISE)):
            over["refill_nothing_finished" + tag] = timed(lambda: arr.refill(m, scen, 0, 400, fl, cs))
            over["refill_one_slot" + tag] = timed(lambda: arr.refill(m, scen, 0, 400, fl, cs), before=lambda: arr.flags[S // 2:S // 2 + 1].fill_(1))
        over["noise_draw_alone"] = timed(lambda: m.noise_draw_dev(S, arr.state, arr.noise, ep_flags=arr.flags, stream=cs))
        over["fused_step"] = timed(lambda: arr.step(m, step_flags, cs))
        over["fused_step_kernel"] = m.kernel_name(S)
    print(json.dumps(dict(per_step_overhead=over)), flush=True)
    measure.write_json(a.out, dict(workload=dict(scenario=scen, seeds=E, slots=S, reps=a.reps, **prob), forms=res, prediction=pred, summary=summary,
                                   per_step_overhead=dict(slots=S, launches=a.launches, **over)))


if __name__ == "__main__":
    main()
