"""The level-0 solve kernels the dispatcher can reach, by the overrides that reach them (test_gpu_every_kernel.py, test_gpu_slack_schedule.py).
Needs a GPU (a handle is opened per combination); no test functions here."""
import itertools


def apply(s, ov):
    """the overrides of a `configs` row on a fresh handle"""
    s.set_lanes_per_stage(ov["lps"]); s.set_waves_per_simd(ov["waves"])
    if ov["lanes"]:
        s.set_lanes_per_instance(ov["lanes"])
    s.set_row_parallel(bool(ov["rowpar"])); s.set_block_riccati(bool(ov["blk2"]))
    if ov["mfma"]:
        s.set_matrix_cores(True)


def configs(mpc_gpu, batch=4, lookahead=True):
    """(N, n_obst, overrides, name) for every distinct kernel name the dispatcher reports for a batch of `batch` instances"""
    seen, out = set(), []
    for N, no in itertools.product((10, 20, 31, 40), (3, 5, 10, 2, 4, 7)):
        for lanes, lps, waves, rowpar, mfma, blk2 in itertools.product((0, 16, 21, 32, 64), (0, 1, 2, 3), (0, 1, 2), (1, 0), (0, 1), (0, 1)):
            if mfma and (lanes != 64 or lps != 1 or not rowpar or blk2 or waves):
                continue
            if not rowpar and (lps != 1 or blk2 or waves):
                continue
            if blk2 and (lps == 1 or lanes or waves == 2):
                continue
            ov = dict(lanes=lanes, lps=lps, waves=waves, rowpar=rowpar, mfma=mfma, blk2=blk2)
            with mpc_gpu.BatchedMpc(N, no, 0.1 * N, max_batch=batch) as s:
                try:
                    apply(s, ov)
                    name = s.kernel_name(batch, lookahead=lookahead)
                except mpc_gpu.MpcError:
                    continue
            if name not in seen:
                seen.add(name); out.append((N, no, ov, name))
    return out
