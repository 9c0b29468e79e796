"""Every sample's chip and phasor of the high-dynamics multicorrelator on the GPU (the cases of tests/corr_hd_cases.py:
hd_anchor_kernel, hd_corr_kernel<FMT>, hd_reduce_kernel, derive_hd_job and hd_plan_upload of corr_hd_kernel.hip).

Impulse sweeps: one batch of jobs per sweep through engine.correlate_host, each job meeting the buffer's only non-zero
sample at its own position n0, so its output is v·phasor[n0]·code_t[n0]; per job and tap |out − ref| ≤ 1e-5·|ref|
against the oracle's plain float sum (exact: one non-zero term).  Dense cases: seeded Gaussian samples, the figure of
test_gpu_corr_coverage.py, max over taps |out − ref| / max(|ref|, ‖x‖₂) ≤ 1e-5 against the oracle with double
accumulation; outputs past n_taps and zero-length jobs exactly zero; the same batch launched twice more gives the
same bits.  Plan reuse: one batch handle through a large, a small, a larger and a high-dynamics-free job set, bit-equal
to fresh handles; one MultiCorrelatorRealCodes handle through three lengths.  Refusals: exactly the oracle's.
tests/test_corr_hd_cases.py shows on the CPU what the table reaches and that the bound has teeth.

The worst figure per sweep and case measured on the MI355X is tabulated in DESIGN.md ("High-dynamics correlator
coverage")."""
import numpy as np
import pytest

import corr_hd_cases as H
from gnss_sim_receiver_amd import abi, engine

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", H.SWEEP_IDS)
def test_impulse_sweep_against_the_oracle(ctx, name):
    s, ref = H.SWEEPS[name], H.sweep_reference(name)
    out = engine.correlate_host(ctx, H.sweep_buffer(s), H.sweep_jobs(s), [H.ramp_code(s.L)])
    e = H.impulse_errs(out, ref, s.n_taps)
    j, t = np.unravel_index(np.argmax(e), e.shape)
    print(f"\ncorr-hd-coverage {name}: {len(s.entries)} jobs × {s.n_taps} taps, worst |out − ref|/|ref| {e.max():.3e} "
          f"at n0 = {s.entries[j][1]}, tap {t}")
    assert np.all(out[:, s.n_taps:] == 0), name
    assert e.max() <= H.TOL, "\n" + H.describe_failures(s, out, ref, H.TOL)


def _check_dense(label, out, ref, jobs):
    e = H.dense_errs(out, ref, jobs)
    print(f"\ncorr-hd-coverage {label}: {len(jobs)} jobs, worst err {e.max():.3e} (job {int(np.argmax(e))})")
    for k, j in enumerate(jobs):
        assert np.all(out[k, j["n_taps"]:] == 0), (label, k)
        if j["n_samples"] == 0:
            assert np.all(out[k] == 0), (label, k)
    assert np.all(np.isfinite(out.view(np.float32))), label
    assert e.max() <= H.TOL, (label, e)


@pytest.mark.parametrize("name", H.DENSE_IDS)
def test_dense_case_against_the_double_accumulation_oracle(ctx, name):
    c = H.DENSE_BY_NAME[name]
    x = H.dense_samples(c.fmt)
    out = engine.correlate_host(ctx, x, c.jobs, H.dense_codes())
    _check_dense(name, out, H.dense_reference(name), c.jobs)
    # the same batch launched twice: the same bits each time, and as the first run's
    buf = ctx.upload(x)
    b = engine.CorrelatorBatch(ctx, len(c.jobs))
    try:
        b.set_jobs(c.jobs, H.DENSE_N_BUF)
        fmt = engine.sample_format(x)
        b.launch(buf, fmt)
        first = b.results()
        b.launch(buf, fmt)
        second = b.results()
    finally:
        b.close()
        buf.free()
    assert first.tobytes() == second.tobytes() == out.tobytes(), name


def test_batch_plan_reuse_is_bit_equal_to_fresh_batches(ctx):
    """hd_plan_upload growing and shrinking job_cap, chunk_cap and anchor_cap across set_jobs calls on one handle."""
    x = H.dense_samples("cf32")
    batches = H.reuse_batches()
    fresh = [engine.correlate_host(ctx, x, jobs, H.dense_codes()) for _, jobs in batches]
    for (label, jobs), out in zip(batches, fresh):
        _check_dense(f"reuse-{label} (fresh)", out, H.dense_reference_of("cf32", jobs), jobs)
    buf = ctx.upload(x)
    b = engine.CorrelatorBatch(ctx, max(len(jobs) for _, jobs in batches))
    try:
        for (label, jobs), want in zip(batches, fresh):
            b.set_jobs(jobs, H.DENSE_N_BUF)
            b.launch(buf, abi.FMT_CF32)
            assert b.results().tobytes() == want.tobytes(), label
    finally:
        b.close()
        buf.free()


def test_channel_handle_reuse_across_lengths(ctx):
    """One MultiCorrelatorRealCodes handle: lengths 4097, 100 and 8193 in turn, the high-dynamics resampler switched
    off and on again in between (the standard pair runs while it is off)."""
    x = H.dense_samples("cf32")
    L, step = 10230, H.DENSE_STEPS[2]
    code = H.ramp_code(L)
    sh = H.shifts_for(-0.5, step, [0, 1, 3])
    mc = engine.MultiCorrelatorRealCodes(ctx)
    mc.init(8193, 3)
    try:
        mc.set_local_code_and_taps(L, code, sh)
        for i, n in enumerate((4097, 100, 8193)):
            j = H.hd_job(n, 3, 2, 2 * i + 1, i)
            j["shifts_chips"][:3] = sh
            o = int(j["sample_offset"])
            args = (float(j["rem_carrier_phase_rad"]), float(j["phase_step_rad"]), float(j["phase_rate_step_rad"]),
                    float(j["rem_code_phase_chips"]), float(j["code_phase_step_chips"]), float(j["code_phase_rate_step_chips"]), n)
            got = np.zeros(3, np.complex64)
            mc.set_input_output_vectors(got, x[o: o + n])
            mc.set_high_dynamics_resampler(False)
            mc.Carrier_wipeoff_multicorrelator_resampler(*args)
            std = got.copy()
            mc.set_high_dynamics_resampler(True)
            mc.Carrier_wipeoff_multicorrelator_resampler(*args)
            jobs = np.array([j], abi.JOB_DTYPE)
            out = np.zeros((1, abi.MAX_TAPS), np.complex64)
            out[0, :3] = got
            _check_dense(f"channel-handle N={n}", out, H.dense_reference_of("cf32", jobs), jobs)
            assert not np.array_equal(std, got), n   # the other kernel pair ran in between
    finally:
        mc.free()


@pytest.mark.parametrize("name", H.REFUSAL_IDS)
def test_refusals_are_the_oracles(ctx, name):
    """E_INVAL with nothing run for what the oracle refuses; what it accepts equals it."""
    job, refused = H.REFUSALS[name]
    x, code = H.refusal_samples(), H.ramp_code(H.REFUSAL_L)
    ctx.set_code(0, code)
    good = H.REFUSALS["shift-equals-N"][0]
    buf = ctx.upload(x)
    b = engine.CorrelatorBatch(ctx, 1)
    try:
        if not refused:
            b.set_jobs(job, H.REFUSAL_N_BUF)
            b.launch(buf, abi.FMT_CF32)
            out = b.results()
            ref = H.DenseReference(H.O.corr_batch(x, job, [code], accum_f64=True), H.C.job_norms(x, job))
            _check_dense(f"accepted {name}", out, ref, job)
            return
        b.set_jobs(good, H.REFUSAL_N_BUF)
        b.launch(buf, abi.FMT_CF32)
        want = b.results()
        with pytest.raises(abi.GnssHipError) as err:
            b.set_jobs(job, H.REFUSAL_N_BUF)
        assert err.value.code == abi.E_INVAL
        b.launch(buf, abi.FMT_CF32)     # a refused job set leaves an empty batch: nothing runs
        b.set_jobs(good, H.REFUSAL_N_BUF)
        b.launch(buf, abi.FMT_CF32)
        assert b.results().tobytes() == want.tobytes()
    finally:
        b.close()
        buf.free()


@pytest.mark.parametrize("n_taps", [0, 9])
def test_channel_handle_refuses_tap_counts(ctx, n_taps):
    mc = engine.MultiCorrelatorRealCodes(ctx)
    with pytest.raises(abi.GnssHipError) as err:
        mc.init(600, n_taps)
    assert err.value.code == abi.E_INVAL


def test_channel_handle_refuses_shifts_beyond_the_length(ctx):
    x = H.refusal_samples()
    mc = engine.MultiCorrelatorRealCodes(ctx)
    mc.init(600, 2)
    try:
        mc.set_high_dynamics_resampler(True)
        mc.set_local_code_and_taps(H.REFUSAL_L, H.ramp_code(H.REFUSAL_L), H.shifts_for(-0.5, 0.25575, [0, 600]))
        got = np.zeros(2, np.complex64)
        mc.set_input_output_vectors(got, x[:600])
        with pytest.raises(abi.GnssHipError) as err:
            mc.Carrier_wipeoff_multicorrelator_resampler(0.4, 0.02, 3e-9, 0.3, 0.25575, -2e-10, 599)   # S = 600 > 599
        assert err.value.code == abi.E_INVAL and np.all(got == 0)
        mc.Carrier_wipeoff_multicorrelator_resampler(0.4, 0.02, 3e-9, 0.3, 0.25575, -2e-10, 600)       # S == N: accepted
        ref = H.O.multicorrelator(x[:600], H.ramp_code(H.REFUSAL_L), H.shifts_for(-0.5, 0.25575, [0, 600]), 0.4, 0.02, 0.3, 0.25575,
                                  n=600, carr_rate=3e-9, code_rate=-2e-10, high_dyn=True)
        assert np.max(np.abs(got - ref) / np.maximum(np.abs(ref), np.linalg.norm(x[:600]))) <= H.TOL
    finally:
        mc.free()
