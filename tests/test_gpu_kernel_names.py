"""mpc_get_kernel_name answers, for every handle state of the sweep of scripts/record_kernel_names.py, what the recorded build answered
(tests/golden/kernel_names.json, kernel_names_bounds.json): the same kernel name, or the same MpcError text.  The name is a formatting of the plan the launch looks its
kernel up with (csrc/solve_dispatch.hpp), so this pins the whole host dispatch -- family, capacity, shape arguments, run-time row count,
feature level, every refusal and its precedence -- across refactors; that the launch runs the kernel the name says is test_gpu_every_kernel.py's part.
Nothing is launched here."""
import importlib.util
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
    cu = rec_mod.compute_units()
    bad = []
    for (golden, features, _), least in zip(rec_mod.RECORDS, (50000, 20000)):      # levels 0 to 3; the states with instance bounds
        rec_cu, rec = rec_mod.load(golden)
        # the crossovers are multiples of the SIMD count: on another device the sweep asks other questions, so the record does not apply (no skip: record it there)
        assert cu == rec_cu, f"this device has {cu} compute units, {os.path.basename(golden)} was recorded on one with {rec_cu}"
        now = rec_mod.sweep(mpc_gpu, cu, features)
        assert list(now) == list(rec)
        total = 0
        for case, want in rec.items():
            assert len(now[case]) == len(want), (case, len(now[case]), len(want))
            total += len(want)
            bad += [(case, k, a, b) for k, (a, b) in enumerate(zip(now[case], want)) if a != b]
        assert total > least, (os.path.basename(golden), total)      # every record by itself
    assert not bad, (len(bad), bad[:10])
