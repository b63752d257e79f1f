"""Case table of the packed-requests net of the factor sweep (test_factor_sweep_requests_host.py, test_gpu_factor_sweep_requests.py).  On the dense
split kernels the sweep fetches row 4 of W~_t from the words of the dead row 5 of the stage's H~aug block (one request with row 4 of H~aug_t) and
stores K~ and the factors 1/d0, l, 1/d1 with one request, the factors from two mirror lanes (rowpar_factor<.., PACKED>, rti_kernel.hpp).  A misplaced
word shows only where the moved words are non-zero and read: row 4 of W~_t carries the affine entry b_t[4], which is zero on a dynamically consistent
start, so every solve here starts from an iterate with seeded uniform noise on X (factor_sweep_live_rows_cases.perturbed, amplitude NOISE = 0.2).

Rows: the smallest horizons at which the two-stage loop's control flow differs -- N = 2: one stage pair, no remainder; N = 3: a pair plus the odd
remainder stage; N = 20, the flagship shape; N = 21 with three obstacles on two lanes per stage.  Batch 8.  The rows have the fields of
factor_sweep_cases.ROWS (off_default_cases.configure and factor_sweep_live_rows_cases.oracle_three_solves read them).  `ok`: the oracle ALONE returns
status 0 below the iteration cap on every instance on all three solves (the host test asserts it)."""
from helpers import random_batch


def _row(id, N, no, seed, Tf, name, B=8):
    return dict(id=id, N=N, no=no, B=B, seed=seed, Tf=Tf, lps=0, lpi=0, waves=0, name=name, ok=(B, B, B))


ROWS = [
    _row("split3-n2", 2, 3, 21, 0.2, "rti_split_kernel<3, 3, false, false, false>"),
    _row("split3-n3", 3, 3, 22, 0.3, "rti_split_kernel<3, 3, false, false, false>"),
    _row("split3-n20", 20, 3, 23, 2.0, "rti_split_kernel<3, 3, false, false, false>"),
    _row("split2-3-n21", 21, 3, 24, 2.1, "rti_split_kernel<3, 2, false, false, false>"),
]
ROW = {r["id"]: r for r in ROWS}

# the closed loop: 10 fused control steps at N = 20 / 3 obstacles, batch 8, velocity noise on the obstacles
LOOP = dict(N=20, no=3, B=8, Tf=2.0, steps=10, seed=25, noise_seed=26, name="rti_split_kernel<3, 3, false, false, false>")

# the family that keeps the sweep's old text against the one that changed, bit for bit: two wavefronts per SIMD (compact blocks) forced at batch 8
W2 = dict(N=20, no=3, B=8, Tf=2.0, seed=27, dense="rti_split_kernel<3, 3, false, false, false>", w2="rti_split_kernel<3, 3, true, false, false>")


def batch(row):
    return random_batch(row["B"], row["no"], seed=row["seed"])
