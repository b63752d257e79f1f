"""Record what mpc_get_kernel_name answers for every handle state of a sweep: tests/golden/kernel_names.json (feature levels 0 to 3) and
tests/golden/kernel_names_bounds.json (the states with instance bounds, level 4: a record of its own, run-length encoded, so that adding it left the first
file byte for byte what it was).

Usage (on the GPU the crossovers were measured on; creating a handle needs a device, naming a kernel launches nothing):
    python scripts/record_kernel_names.py [OUT_DIRECTORY]
The record pins the host dispatcher across refactors: tests/test_gpu_kernel_names.py replays `sweep()` on the current build and compares every
entry -- a kernel name, or the text of the MpcError the call (or a setter in front of it) raised.  Run it on the commit whose answers are to be kept.

The sweep: N x n_obst (mpc_create up to 10 obstacles, mpc_create2 beyond, where N = 40 must refuse) x feature state x the override product of
tests/test_gpu_every_kernel.py::_configs x batch sizes on either side of every crossover of pick_lanes / pick_split / pick_waves (multiples of the
device's SIMD count, which is why the record carries the compute-unit count) x look-ahead both ways at N = 40 (the compact / dense LDS decision).
Entries are indices into one list of distinct strings, in sweep order; in a run-length encoded record ("rle": true) [index, count] pairs.
"""
import ctypes as C
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dynamic-obstacle-avoidance-mpc_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_names.json")
HORIZONS = (10, 20, 31, 40)
OBST_CREATE, OBST_CREATE2 = (2, 3, 4, 5, 7, 10), (11, 15, 20, 25, 32)
GOLDEN_BOUNDS = os.path.join(ROOT, "tests", "golden", "kernel_names_bounds.json")
FEATURES = ("none", "reference", "instance parameters", "obstacle mask", "mask + parameters + reference")
FEATURES_BOUNDS = ("instance bounds", "bounds + mask + parameters + reference")
RECORDS = ((GOLDEN, FEATURES, False), (GOLDEN_BOUNDS, FEATURES_BOUNDS, True))      # (file, feature states, run-length encoded)
MAX_BATCH = 4


def cases():
    """(N, n_obst, creating entry point)"""
    out = [(N, no, "mpc_create") for N in HORIZONS for no in OBST_CREATE]
    out += [(N, no, "mpc_create2") for N in HORIZONS if N <= 31 for no in OBST_CREATE2]
    return out + [(40, 15, "mpc_create2")]


def overrides():
    """the override product of tests/test_gpu_every_kernel.py::_configs"""
    out = []
    for lanes, lps, waves, rowpar, mfma, blk2 in itertools.product((0, 16, 21, 32, 64), (0, 1, 2, 3), (0, 1, 2), (1, 0), (0, 1), (0, 1)):
        if mfma and (lanes != 64 or lps != 1 or not rowpar or blk2 or waves):
            continue
        if not rowpar and (lps != 1 or blk2 or waves):
            continue
        if blk2 and (lps == 1 or lanes or waves == 2):
            continue
        out.append((lanes, lps, waves, rowpar, mfma, blk2))
    return out


def batches(simd_count):
    return (4, 4 * simd_count + 1, 7 * simd_count + 1, 8 * simd_count + 1, 12 * simd_count + 1, 65536)


def _open(mpc_gpu, N, no, create):
    """a BatchedMpc whose handle comes from the named entry point.  BatchedMpc.__init__ always calls mpc_create2, so the object is made without it and
    given the attributes __init__ sets; only the setters, kernel_name and close are used on it (a field added to BatchedMpc that those read belongs here too)"""
    from mpc_gpu import _lib
    s = mpc_gpu.BatchedMpc.__new__(mpc_gpu.BatchedMpc)
    s.cfg = _lib.default_config(N, no, 0.1 * N)
    s.N, s.n_obst, s.Tf, s.dt, s.max_batch, s.device = N, no, 0.1 * N, 0.1, MAX_BATCH, 0
    s._h = C.c_void_p()
    _lib.check(getattr(_lib.lib(), create)(C.byref(s.cfg), 0, MAX_BATCH, C.byref(s._h)))
    return s


def _set_feature(s, feature):
    s.set_reference(None); s.set_instance_params(); s.set_obstacle_mask(None); s.set_instance_bounds()
    if "reference" in feature:
        s.set_reference(np.zeros((MAX_BATCH, s.N + 1, 6)))
    if "parameters" in feature:
        s.set_instance_params(W=np.ones((MAX_BATCH, 6)))
    if "mask" in feature:
        s.set_obstacle_mask(np.ones((MAX_BATCH, s.n_obst), dtype=bool))
    if "bounds" in feature:      # the handle's own values
        s.set_instance_bounds(bx_lo=list(s.cfg.bx_lo), bx_hi=list(s.cfg.bx_hi), bu_lo=list(s.cfg.bu_lo), bu_hi=list(s.cfg.bu_hi))


def _set_overrides(s, lanes, lps, waves, rowpar, mfma, blk2):
    s.set_lanes_per_stage(0); s.set_waves_per_simd(0); s.set_lanes_per_instance(0)
    s.set_row_parallel(True); s.set_block_riccati(False); s.set_matrix_cores(False)
    s.set_lanes_per_stage(lps); s.set_waves_per_simd(waves)
    if lanes:
        s.set_lanes_per_instance(lanes)
    s.set_row_parallel(bool(rowpar)); s.set_block_riccati(bool(blk2))
    if mfma:
        s.set_matrix_cores(True)


def sweep(mpc_gpu, cu_count, features=FEATURES):
    """{"N n_obst entry_point": [entry, ...]}: the answers in sweep order.  A refused creation or a refused setter is ONE entry, its error text."""
    out = {}
    for N, no, create in cases():
        entries = out.setdefault(f"{N} {no} {create}", [])
        try:
            s = _open(mpc_gpu, N, no, create)
        except mpc_gpu.MpcError as e:
            entries.append(str(e))
            continue
        with s:
            for feature in features:
                _set_feature(s, feature)
                for ov in overrides():
                    try:
                        _set_overrides(s, *ov)
                    except mpc_gpu.MpcError as e:
                        entries.append(str(e))
                        continue
                    for batch, lookahead in itertools.product(batches(4 * cu_count), (True, False) if N == 40 else (True,)):
                        try:
                            entries.append(s.kernel_name(batch, lookahead=lookahead))
                        except mpc_gpu.MpcError as e:
                            entries.append(str(e))
    return out


def compute_units():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def load(path):
    """(compute units, {case: [entry, ...]}) of a record, either encoding"""
    with open(path) as f:
        rec = json.load(f)
    if rec.get("rle"):
        cases = {c: [rec["strings"][k] for k, n in runs for _ in range(n)] for c, runs in rec["cases"].items()}
    else:
        cases = {c: [rec["strings"][k] for k in idx] for c, idx in rec["cases"].items()}
    return rec["compute_units"], cases


def dump(path, cu, answers, rle):
    strings = sorted({e for v in answers.values() for e in v})
    index = {e: k for k, e in enumerate(strings)}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        if not rle:
            json.dump({"compute_units": cu, "strings": strings, "cases": {k: [index[e] for e in v] for k, v in answers.items()}}, f, separators=(",", ":"))
            f.write("\n")
            return strings
        lines = []      # one case per line: a re-record changes the lines of the cases that changed
        for case, v in answers.items():
            runs = []
            for e in v:
                if runs and runs[-1][0] == index[e]:
                    runs[-1][1] += 1
                else:
                    runs.append([index[e], 1])
            lines.append(f"{json.dumps(case)}:{json.dumps(runs, separators=(',', ':'))}")
        f.write('{"compute_units":%d,"rle":true,\n"strings":[\n%s],\n"cases":{\n%s}}\n' % (cu, ",\n".join(json.dumps(e) for e in strings), ",\n".join(lines)))
    return strings


def against_previous(old_cases, answers):
    """What a re-record changes, before the file is overwritten: (entries that answer what they did, [(case, position, before, now)] of those that do not,
    counting a changed length as one)"""
    kept, changed = 0, []
    for case, want in old_cases.items():
        now = answers.get(case, [])
        if len(now) != len(want):
            changed.append((case, -1, len(want), len(now)))
            continue
        kept += sum(a == b for a, b in zip(now, want))
        changed += [(case, k, b, a) for k, (a, b) in enumerate(zip(now, want)) if a != b]
    return kept, changed


def main(out_dir=None):
    import mpc_gpu
    mpc_gpu.build()
    cu = compute_units()
    for golden, features, rle in RECORDS:
        path = golden if out_dir is None else os.path.join(out_dir, os.path.basename(golden))
        answers = sweep(mpc_gpu, cu, features)
        if os.path.exists(golden):
            old_cu, old_cases = load(golden)
            if old_cu == cu:
                kept, changed = against_previous(old_cases, answers)
                print(f"{os.path.basename(golden)}: {kept} entries of {len(old_cases)} recorded cases answer what they did, {len(changed)} do not", changed[:5])
        strings = dump(path, cu, answers, rle)
        print(f"{path}: {sum(len(v) for v in answers.values())} entries, {len(strings)} distinct, {len(answers)} cases, {cu} compute units")
        for e in strings:
            print("   ", e)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
