"""Record what mpc_get_kernel_name answers for every handle state of a sweep: tests/golden/kernel_names.json.

Usage (on the GPU the crossovers were measured on; creating a handle needs a device, naming a kernel launches nothing):
    python scripts/record_kernel_names.py [OUT.json]
The record pins the host dispatcher across refactors: tests/test_gpu_kernel_names.py replays `sweep()` on the current build and compares every
entry -- a kernel name, or the text of the MpcError the call (or a setter in front of it) raised.  Run it on the commit whose answers are to be kept.

The sweep: N x n_obst (mpc_create up to 10 obstacles, mpc_create2 beyond, where N = 40 must refuse) x feature state x the override product of
tests/test_gpu_every_kernel.py::_configs x batch sizes on either side of every crossover of pick_lanes / pick_split / pick_waves (multiples of the
device's SIMD count, which is why the record carries the compute-unit count) x look-ahead both ways at N = 40 (the compact / dense LDS decision).
Entries are indices into one list of distinct strings, in sweep order.
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
FEATURES = ("none", "reference", "instance parameters", "obstacle mask", "mask + parameters + reference")
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
    s.set_reference(None); s.set_instance_params(); s.set_obstacle_mask(None)
    if "reference" in feature:
        s.set_reference(np.zeros((MAX_BATCH, s.N + 1, 6)))
    if "parameters" in feature:
        s.set_instance_params(W=np.ones((MAX_BATCH, 6)))
    if "mask" in feature:
        s.set_obstacle_mask(np.ones((MAX_BATCH, s.n_obst), dtype=bool))


def _set_overrides(s, lanes, lps, waves, rowpar, mfma, blk2):
    s.set_lanes_per_stage(0); s.set_waves_per_simd(0); s.set_lanes_per_instance(0)
    s.set_row_parallel(True); s.set_block_riccati(False); s.set_matrix_cores(False)
    s.set_lanes_per_stage(lps); s.set_waves_per_simd(waves)
    if lanes:
        s.set_lanes_per_instance(lanes)
    s.set_row_parallel(bool(rowpar)); s.set_block_riccati(bool(blk2))
    if mfma:
        s.set_matrix_cores(True)


def sweep(mpc_gpu, cu_count):
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
            for feature in FEATURES:
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


def main(path):
    import mpc_gpu
    mpc_gpu.build()
    cu = compute_units()
    answers = sweep(mpc_gpu, cu)
    strings = sorted({e for v in answers.values() for e in v})
    index = {e: k for k, e in enumerate(strings)}
    rec = {"compute_units": cu, "strings": strings, "cases": {k: [index[e] for e in v] for k, v in answers.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print(f"{path}: {sum(len(v) for v in answers.values())} entries, {len(strings)} distinct, {len(answers)} cases, {cu} compute units")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
