"""The measurement protocol of the scripts/*_rate.py programs, in one place: the path prelude, the GPU requirement, a stream of one's own, the HIP event
window, the rep loop (a dropped warm-up rep, the forms alternating rep by rep), median and spread, the two merges of a result JSON, and the A/B run of
bench.py against the parent commit's library.  Plain Python and numpy; torch is imported by require_gpu() or handed in by the caller, so everything here
but require_gpu() runs -- and is tested, tests/test_measure_host.py -- without a device.

    import measure                      # a rate script runs as scripts/<name>.py, so scripts/ is on the path already
    torch = measure.require_gpu()
    with measure.own_stream(torch) as st:
        ms = measure.alternate({"form": lambda: measure.window(torch, st, body, launches, prepare)}, reps)
    median, spread = measure.summary(ms["form"])
"""
import contextlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dynamic-obstacle-avoidance-mpc_amd"), os.path.join(ROOT, "tests")]


def require_gpu():
    """torch, with a device behind it; a rate script has no other way to run"""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures on the device only")
    return torch


def _own(stream):
    # The library reads a stream handle of 0 as "the handle's own stream": with torch's legacy default stream (handle 0) the launches would go to another
    # stream than the events around them, and the events would time the enqueue only.
    if stream.cuda_stream == 0:
        raise ValueError("a measurement needs a stream of its own: handle 0 is the library's word for the handle's own stream")
    return stream


@contextlib.contextmanager
def own_stream(torch, stream=None, device=0):
    """`stream` (default: a new stream on `device`) as torch's current stream; the default stream is refused"""
    st = _own(stream if stream is not None else torch.cuda.Stream(device=torch.device("cuda", device)))
    with torch.cuda.stream(st):
        yield st


def window(torch, stream, body, launches, prepare=None):
    """milliseconds per launch of `launches` back-to-back body() between two HIP events on `stream`: prepare(), device synchronise, record, the launches,
    record, device synchronise -- the set-up has run and the device is idle when the first event is recorded"""
    _own(stream)
    if prepare:
        prepare()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    for _ in range(launches):
        body()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def per_call(torch, stream, body, launches, prepare=None):
    """median, minimum and maximum in microseconds over `launches` windows of ONE body() each (prepare() in front of each, outside its window); between
    them the stream is synchronised, not the device"""
    _own(stream)
    ms = []
    for _ in range(launches):
        if prepare:
            prepare()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); body(); e1.record(stream)
        stream.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median_us=1e3 * float(np.median(ms)), min_us=1e3 * float(np.min(ms)), max_us=1e3 * float(np.max(ms)))


def wall(call, torch=None):
    """(seconds on the wall clock, call()'s result); with torch: device synchronise, clock, call, device synchronise.  Without it the call must end in a
    synchronise of its own."""
    if torch:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = call()
    if torch:
        torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def alternate(forms, reps, on_run=None):
    """{form: [what its callable returned in reps 1 .. reps]}: reps + 1 passes over the forms in the mapping's order, so that the forms alternate and a drift
    of the machine meets all of them; rep 0 warms every form up and is dropped.  on_run(rep, form, value) sees every run, rep 0 included."""
    if reps < 1:
        raise ValueError(f"reps = {reps}: rep 0 is the warm-up, at least one more is needed")
    values = {f: [] for f in forms}
    for rep in range(reps + 1):
        for f, fn in forms.items():
            v = fn()
            if rep:
                values[f].append(v)
            if on_run:
                on_run(rep, f, v)
    return values


def summary(values):
    """(median, spread): spread = (max - min) / median"""
    med = float(np.median(values))
    return med, float((max(values) - min(values)) / med)


def summaries(values):
    """({form: median}, {form: spread}) of alternate()'s result"""
    s = {f: summary(v) for f, v in values.items()}
    return {f: m for f, (m, _) in s.items()}, {f: sp for f, (_, sp) in s.items()}


def read_json(path):
    """a part-merged result as it stands ({} before the first run): a script replaces the parts it ran and writes the rest back with write_json()"""
    if os.path.exists(path):
        with open(path) as f:
            return json.load(f)
    return {}


def write_json(path, result):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)


def merge_cells(path, header, rows, order, extra=None):
    """writes dict(**header, cells=..., **extra): `rows` beside the file's other cells, in the order of the cell names `order`.  The file's cells are kept
    only if its header fields equal `header` (cells measured otherwise do not mix); an `extra` entry that is None keeps the file's value whatever the header."""
    prev = read_json(path)
    old = []
    if all(prev.get(k) == v for k, v in header.items()):
        old = [c for c in prev.get("cells", []) if c["cell"] not in {r["cell"] for r in rows}]
    extra = {k: prev.get(k) if v is None else v for k, v in (extra or {}).items()}
    write_json(path, dict(header, cells=sorted(old + rows, key=lambda c: order.index(c["cell"])), **extra))


def bench_ab(parent_lib, rounds, this_first=False, run=subprocess.run):
    """bench.py --gpus 1 --steps 20 --warmup 5 with the parent commit's library (handed to the run as MPC_GPU_LIB) and this one's, alternating `rounds`
    times, parent first (this_first: the other order, to tell a difference between the libraries from one between first and second run of a pair); each
    run a process of its own under a time limit, and nothing is started behind a run that failed"""
    if not parent_lib or not os.path.exists(parent_lib):
        raise SystemExit("the bench.py part needs --parent-lib PATH (a libmpcgpu.so built from the parent commit)")
    runs = []
    for rnd in range(rounds):
        pair = [("parent", os.path.abspath(parent_lib)), ("this", None)]
        for side, lib in (pair[::-1] if this_first else pair):
            env = dict(os.environ)
            env.pop("MPC_GPU_LIB", None)
            if lib:
                env["MPC_GPU_LIB"] = lib
            p = run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], env=env, cwd=ROOT,
                    capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                raise SystemExit(f"bench.py ({side}, round {rnd}) ended with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            line = json.loads(p.stdout.strip().splitlines()[-1])
            runs.append(dict(side=side, round=rnd, value=line.get("value"), unit=line.get("unit"), ms_per_step=line.get("ms_per_step"),
                             mean_ipm_iters=(line.get("config") or {}).get("mean_ipm_iters")))
            print(json.dumps(runs[-1]), flush=True)
    med = {s: float(np.median([r["value"] for r in runs if r["side"] == s])) for s in ("parent", "this")}
    par = [r["value"] for r in runs if r["side"] == "parent"]
    return dict(command="bench.py --gpus 1 --steps 20 --warmup 5", order="this, parent" if this_first else "parent, this", runs=runs, median=med,
                this_over_parent=med["this"] / med["parent"], parent_spread=(max(par) - min(par)) / med["parent"])
