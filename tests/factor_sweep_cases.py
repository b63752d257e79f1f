"""Case table of the factor-sweep net (test_factor_sweep_terms_host.py, test_gpu_factor_sweep_terms.py): the kernels that run rowpar_factor or one of its
one-block twins (rti_kernel.hpp), at the smallest horizons at which the sweep's control flow differs -- N = 2: one trip of the two-stage loop and no
tail; N = 3: one trip and the single-stage tail; N = 20; N = 21 on two lanes per stage -- and one row at dt = 0.15, so that a step handed to the sweep
that is not the W~[3][6] = W~[4][7] the owner lanes stage would show.  The rows have the fields of off_default_cases.ROWS (configure() reads them);
inputs are helpers.random_batch with the row's seed.  `ok`: instances with status 0 on three consecutive solves by the oracle ALONE (a cold start, two
from its own shifted iterate) -- the whole batch in every row, so nothing is left to adjudicate for a reason the GPU has no part in; the host test
asserts it."""
from helpers import random_batch


def _row(id, N, no, B, seed, Tf, lps, lpi, name):
    return dict(id=id, N=N, no=no, B=B, seed=seed, Tf=Tf, lps=lps, lpi=lpi, waves=0, name=name, ok=(B, B, B))


ROWS = [
    # rowpar_factor on the dense stage blocks of the stage-split kernel
    _row("split3-n2", 2, 3, 8, 1, 0.2, 0, 0, "rti_split_kernel<3, 3, false, false, false>"),
    _row("split3-n3", 3, 3, 8, 2, 0.3, 0, 0, "rti_split_kernel<3, 3, false, false, false>"),
    _row("split3-n20-dt", 20, 3, 8, 3, 3.0, 0, 0, "rti_split_kernel<3, 3, false, false, false>"),      # dt = 0.15
    _row("split2-10-n21", 21, 10, 8, 4, 2.1, 0, 0, "rti_split_kernel<10, 2, false, false, false>"),
    # one lane per stage on dense blocks (sweep variant 2)
    _row("g16-n2", 2, 3, 8, 5, 0.2, 1, 16, "rti_solve_kernel<3, 16, 2, false>"),
    _row("g64-n3", 3, 3, 8, 6, 0.3, 1, 64, "rti_solve_kernel<3, 64, 2, false>"),
    # ... and on compact blocks (variant 3: the one-block twin with the reordered terms); 47 stages are the first odd horizon whose dense blocks no
    # longer fit four wavefronts per CU with or without the look-ahead positions (plan_solve)
    _row("g21-n20", 20, 3, 8, 7, 2.0, 1, 21, "rti_solve_kernel<3, 21, 3, false>"),
    _row("compact-n47", 47, 3, 8, 8, 4.7, 1, 64, "rti_solve_kernel<3, 64, 3, false>"),
    # the multi-wavefront kernel
    _row("wide20-n3", 3, 11, 8, 9, 0.3, 0, 0, "rti_wide_kernel<20, 2, true>"),
]
ROW = {r["id"]: r for r in ROWS}


def batch(row):
    return random_batch(row["B"], row["no"], seed=row["seed"])
