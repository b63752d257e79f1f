"""The interior-point trace rule of ip_trace_cases.py proven on the reference alone -- the conditions test_gpu_ip_trace.py relies on:
  calibration  a second rounding of the same arithmetic (the oracle's source built with FMA contraction) stays inside the band on every entry;
  sharpness    a constant of the interior point changed in the sixth or seventh digit leaves the band on every instance -- while the solve ends
               within the parity tolerance after the same number of iterations, which is all helpers.judge_against_oracle looks at;
  caps         every case of the GPU file compares nearly all of the oracle's rows, with few tolerances too loose to mean anything, on solves long
               and damped enough to exercise the centring and the step rule;
  determinism  the band of a case is a function of the case alone.
Artefacts go to build/ip_trace/ (git-ignored) and are reused while they are newer than their sources."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import ip_trace_cases as it

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "build", "ip_trace")
CONTRACTED = ["-O3", "-march=native", "-ffp-contract=fast"]      # the checker itself is -O2 -ffp-contract=off (oracle/Makefile)


@pytest.fixture(scope="module")
def orc(built):
    from oracle import oracle
    return oracle


def _stale(target, sources):
    return not os.path.exists(target) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in sources)


def _contracted_library():
    os.makedirs(OUT, exist_ok=True)
    src = [os.path.join(ROOT, "oracle", f) for f in ("mpc_oracle.c", "mpc_oracle.h")]
    so = os.path.join(OUT, "liborc_contracted.so")
    if _stale(so, src):
        tmp = f"{so}.{os.getpid()}.new"
        subprocess.check_call([os.environ.get("CC", "gcc"), *CONTRACTED, "-fPIC", "-fopenmp", "-std=c11", "-shared", "-o", tmp, src[0], "-lm"])
        os.replace(tmp, so)
    return so


def _as_rows(results):
    rows = np.zeros((len(results), max([r["iters"] for r in results] + [1]), 4))
    for k, r in enumerate(results):
        rows[k, :r["iters"]] = r["trace"]
    return rows, [r["iters"] for r in results]


def test_calibration_a_second_rounding_stays_inside_the_band(orc):
    """the oracle's source with FMA contraction, loaded in a child process (the checker of this process is never switched), on the sample of 112
    instances: every entry inside max(FLOOR, MARGIN * spread), every iteration count equal.  Measured where this was written: 1073 rows, no
    trace bitwise equal, worst err / tol 0.50 (alpha, the floor's own jump), 21 of 4292 tolerances beyond 1e-4"""
    problems = it.sample(orc)
    assert sum(len(p["x0"]) for _, p in problems) == 112
    so = _contracted_library()
    fin, fout = os.path.join(OUT, f"sample.{os.getpid()}.in"), os.path.join(OUT, f"sample.{os.getpid()}.out")
    with open(fin, "wb") as f:
        pickle.dump(it.pack(problems), f)
    try:
        subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ip_trace_cases.py"), so, fin, fout], check=True, timeout=600)
        with open(fout, "rb") as f:
            other = dict(pickle.load(f))
    finally:
        for p in (fin, fout):
            if os.path.exists(p):
                os.remove(p)
    total, equal, instances = {}, 0, 0
    report = []
    for name, p in problems:
        bands = it.band_of(orc, p)
        rows, iters = _as_rows(other[name])
        j = it.judge_trace(rows, iters, bands)
        it.merge(total, j)
        equal += sum(np.array_equal(r["trace"], b["trace"]) for r, b in zip(other[name], bands)); instances += len(bands)
        report.append((name, j["worst"], j["rows"], j["loose"], j["first"], [r["iters"] for r in other[name]] == [b["iters"] for b in bands]))
    print(f"IP-TRACE calibration: {instances} instances, {total['rows']} rows, {equal} traces bitwise equal, worst err / tol {total['worst']:.3f}, "
          f"{total['loose']} of {total['entries']} tolerances beyond {it.LOOSE}: {report}")
    if equal == instances:
        pytest.skip("no trace of the contracted build differs bitwise from the checker's: this host contracts nothing (no FMA), the calibration says nothing here")
    assert all(ok for *_, ok in report), report                                  # every iteration count equal
    assert total["offending"] == 0 and total["worst"] <= 1.0, report            # every entry inside the rule
    assert total["rows"] >= 0.95 * total["oracle_rows"]


def test_sharpness_what_the_end_point_comparison_cannot_see(orc):
    """mu0 and thr0 scaled by 1 + 1e-6, slack_b by 1 + 1e-7: X and U move by less than the parity tolerance and the iteration counts stay -- and
    the trace leaves the band on every instance"""
    seen = []
    for name, p in it.mutant_sample(orc):
        bands = it.band_of(orc, p)
        for field, rel in it.MUTANTS:
            cm = it.mutated(orc, p["cfg"], field, rel)
            assert getattr(cm, field) != getattr(p["cfg"], field)
            for b, band in enumerate(bands):
                r = orc.rti_solve_trace(cm, p["x0"][b], p["P"][b], p["goal"][b], p["X"][b], p["U"][b])
                j = it.judge_trace(r["trace"][:r["iters"]], r["iters"], band)
                moved = max(np.abs(r["X"] - band["X"]).max(), np.abs(r["U"] - band["U"]).max())
                # what judge_against_oracle would see: nothing
                assert r["status"] == band["status"] and r["iters"] == band["iters"] and moved <= 1e-6, (name, field, b, r["iters"], band["iters"], moved)
                # what the trace sees
                assert j["first"] is not None, (name, field, b, j)
                seen.append((name, field, j["offending"] / j["entries"], moved))
    assert len(seen) == len(it.MUTANT_SHAPES) * len(it.MUTANTS) * it.SAMPLE_B
    for field, _ in it.MUTANTS:
        f = [s[2] for s in seen if s[1] == field]
        print(f"IP-TRACE sharpness {field}: caught on {len(f)} of {len(f)} instances, {min(f):.0%} .. {max(f):.0%} of their entries; "
              f"largest |dX|, |dU| {max(s[3] for s in seen if s[1] == field):.2e}")


_CASES = {}


def _gpu_cases(orc):
    if not _CASES:
        for cid, bands, exempt in it.gpu_cases(orc):
            _CASES[cid] = (bands, exempt)
    return _CASES


def test_caps_every_gpu_case_is_long_tight_and_damped_enough(orc):
    bad = []
    cases = _gpu_cases(orc)
    assert len(cases) >= 100
    for cid, (bands, exempt) in cases.items():
        c = it.conditions(bands)
        why = []
        if c["worst"] != 0.0: why.append("the checker's own trace is not at the centre of its band")
        if c["compared"] < 0.95 * c["oracle_rows"]: why.append(f"rows compared {c['compared']} of {c['oracle_rows']}")
        if c["loose"] > 0.02 * c["entries"]: why.append(f"{c['loose']} of {c['entries']} tolerances beyond {it.LOOSE}")
        if not exempt:
            if c["longest"] < 8: why.append(f"longest solve {c['longest']} rows")
            if not c["damped"]: why.append("no instance with alpha < 1")
            if not c["centred"]: why.append("no instance with sigma > 0.1")
        if why:
            bad.append((cid, why))
    print(f"IP-TRACE caps: {len(cases)} cases, {sum(it.conditions(b)['compared'] for b, _ in cases.values())} rows")
    assert not bad, bad


def test_determinism_the_band_is_a_function_of_the_case(orc):
    p = it.cold(orc, 20, 3, 4)
    a = it.band_of(orc, p)
    it._BANDS.clear()
    b = it.band_of(orc, dict(p, x0=p["x0"].copy(), X=p["X"].copy()))
    for x, y in zip(a, b):
        assert x is not y and np.array_equal(x["trace"], y["trace"]) and np.array_equal(x["spread"], y["spread"]) and x["draw_iters"] == y["draw_iters"]
    assert it.band_of(orc, p)[0] is b[0]                                         # memoised per distinct problem
    assert any(s["spread"].any() for s in b)                                     # the draws do move the trace
    c = it.band_of(orc, p, seed=1)
    assert not all(np.array_equal(x["spread"], y["spread"]) for x, y in zip(b, c))      # another family of draws is another band
    assert all(np.array_equal(x["trace"], y["trace"]) for x, y in zip(b, c))
