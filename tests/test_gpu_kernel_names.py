"""mpc_get_kernel_name answers, for every handle state of the sweep of scripts/record_kernel_names.py, what the recorded build answered
(tests/golden/kernel_names.json): the same kernel name, or the same MpcError text.  The name is a formatting of the plan the launch looks its
kernel up with (csrc/solve_dispatch.hpp), so this pins the whole host dispatch -- family, capacity, shape arguments, run-time row count,
feature level, every refusal and its precedence -- across refactors; that the launch runs the kernel the name says is test_gpu_every_kernel.py's part.
Nothing is launched here."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_kernel_names", os.path.join(ROOT, "scripts", "record_kernel_names.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_name_and_refusal_is_the_recorded_one(built):
    import mpc_gpu
    rec_mod = _recorder()
    with open(rec_mod.GOLDEN) as f:
        rec = json.load(f)
    cu = rec_mod.compute_units()
    # the crossovers are multiples of the SIMD count: on another device the sweep asks other questions, so the record does not apply (no skip: record it there)
    assert cu == rec["compute_units"], f"this device has {cu} compute units, tests/golden/kernel_names.json was recorded on one with {rec['compute_units']}"
    now = rec_mod.sweep(mpc_gpu, cu)
    assert list(now) == list(rec["cases"])
    total, bad = 0, []
    for case, idx in rec["cases"].items():
        want = [rec["strings"][k] for k in idx]
        assert len(now[case]) == len(want), (case, len(now[case]), len(want))
        total += len(want)
        bad += [(case, k, a, b) for k, (a, b) in enumerate(zip(now[case], want)) if a != b]
    assert total > 50000, total
    assert not bad, (len(bad), bad[:10])
