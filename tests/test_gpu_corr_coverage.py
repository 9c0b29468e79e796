"""Every sample format, tap class, margin state and work-item shape of the batched correlator on the GPU (the cases
of tests/corr_cases.py: corr_batch_kernel's 48 instantiations, the host plan around it, the 16384-chip launch).

Per case, one small batch through engine.correlate_host.  Per job  err = max over taps |out − ref| / max(|ref|, ‖x‖₂)
against the oracle with double accumulation on the same (unscaled) samples, ‖x‖₂ over the job's own samples: err ≤ 1e-5,
the project's contract (BASELINE.json north star).  Zero-length jobs and outputs past n_taps are exactly zero; the same
batch launched twice more gives the same bits.  tests/test_corr_cases.py shows on the CPU what the reference and the
bound are worth (headroom, sensitivity) and that the table reaches every instantiation.

The worst err per class and format measured on the MI355X is tabulated in DESIGN.md ("Batched correlator coverage")."""
import numpy as np
import pytest

import corr_cases as C
from gnss_sim_receiver_amd import abi, engine

pytestmark = pytest.mark.gpu


def _check(name, out, label=""):
    c, r = C.BY_NAME[name], C.reference(name)
    e = C.job_errs(out, r.ref, r.norms, c.jobs)
    print(f"\ncorr-coverage {name}{label}: reaches {sorted(c.reaches)} worst err {e.max():.3e}")
    for k, j in enumerate(c.jobs):
        assert np.all(out[k, j["n_taps"]:] == 0), (name, k)
        if j["n_samples"] == 0:
            assert np.all(out[k] == 0), (name, k)
    assert np.all(np.isfinite(out.view(np.float32))), name
    assert e.max() <= C.TOL, (name, e)


@pytest.mark.parametrize("name", C.CASE_IDS)
def test_case_against_the_double_accumulation_oracle(ctx, monkeypatch, name):
    c = C.BY_NAME[name]
    for k, v in c.env.items():  # read by set_jobs
        monkeypatch.setenv(k, v)
    x = C.samples(c.fmt)
    out = engine.correlate_host(ctx, x, c.jobs, list(C.codes()))
    _check(name, out)
    # the same batch launched twice: the same bits each time, and as the first run's
    buf = ctx.upload(x)
    b = engine.CorrelatorBatch(ctx, len(c.jobs))
    try:
        b.set_jobs(c.jobs, C.N_BUF)
        fmt = engine.sample_format(x)
        b.launch(buf, fmt)
        first = b.results()
        b.launch(buf, fmt)
        second = b.results()
    finally:
        b.close()
        buf.free()
    assert first.tobytes() == second.tobytes() == out.tobytes(), name


@pytest.mark.parametrize("n", [4097, 16385])
def test_reference_class_avx_single_job_plan(ctx, n):
    """MultiCorrelatorRealCodes with the AVX rotator: the pair_by_code = false plan of one job (an item of 2 chunks;
    an item of 4 and an item of 1)."""
    name = f"len{n}-avx-cf32"
    j = C.BY_NAME[name].jobs[0]
    t = int(j["n_taps"])
    x = C.samples("cf32")[int(j["sample_offset"]): int(j["sample_offset"]) + n]
    mc = engine.MultiCorrelatorRealCodes(ctx, rotator=abi.ROTATOR_AVX)
    mc.init(n, t)
    try:
        mc.set_local_code_and_taps(C.L_MAIN, C.codes()[C.MAIN], j["shifts_chips"][:t])
        got = np.zeros(t, np.complex64)
        mc.set_input_output_vectors(got, x)
        mc.Carrier_wipeoff_multicorrelator_resampler(float(j["rem_carrier_phase_rad"]), float(j["phase_step_rad"]), 0.0,
                                                     float(j["rem_code_phase_chips"]), float(j["code_phase_step_chips"]), 0.0, n)
    finally:
        mc.free()
    out = np.zeros((1, abi.MAX_TAPS), np.complex64)
    out[0, :t] = got
    _check(name, out, " (MultiCorrelatorRealCodes)")
