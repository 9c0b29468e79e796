"""Galileo E5a / E5b PCPS acquisition (engine.galileo_e5a_pcps_acquisition, engine.galileo_e5b_pcps_acquisition:
the two adapters' parameters) on the device vs the oracle's acquisition_core restatement.

  5I, 5Q, 5X   12.5 Msps, a 12500-sample search (1 ms), ±2000 Hz in 250 Hz steps
  7X           10 Msps (GALILEO_E5B_OPT_ACQ_FS_SPS, the resampler's target), a 10000-sample search

Every signal carries both components, (d·sec_I·c_I + j·sec_Q[prn]·c_Q)/√2: the single-component searches see the
other component as cross-correlation noise, the X search (I chips in the real part, Q chips in the imaginary part
of the local code) collects both.  The block spans two code periods over which the secondary codes of both
components of every present PRN keep one sign (found below: a secondary-chip flip inside a 1 ms circular
correlation splits the peak, which is a property of the signal and not of either implementation).

(bin, index), acq_delay_samples and doppler_hz are compared exactly — the oracle's peak / second-largest margin is
asserted above 1 + 1e-4 — and the statistic within the 2e-3 the B3I / L2C acquisition test uses."""
import numpy as np
import pytest

from gnss_sim_receiver_amd import codes, engine, signals
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TIE = 1.0 + 1e-4
ABSENT = 17
SEED = 31
PRESENT = ((9, -1210.0, 4321.7), (30, 640.0, 9001.2))  # PRN, Doppler, delay in chips
CASES = {  # signal id: band, fs, acquire_pilot, acquire_iq
    "5I": ("a", 12500000, False, False), "5Q": ("a", 12500000, True, False), "5X": ("a", 12500000, True, True),  # acquire_iq overrides
    "7X": ("b", 10000000, False, True),
}


def steady_period(band):
    """The first code period p ≥ 1 such that periods p and p + 1 carry one and the same sign on both components of
    every present PRN (components of opposite sign cancel in the X search: conj(c_I + j·c_Q)·(a·c_I + j·b·c_Q) sums to
    (a + b)·L)."""
    system, _, i_sec, q_sec = {"a": ("GAL_E5A", None, codes.GALILEO_E5A_I_SECONDARY_CODE, codes.galileo_e5a_q_secondary),
                               "b": ("GAL_E5B", None, codes.GALILEO_E5B_I_SECONDARY_CODE, codes.galileo_e5b_q_secondary)}[band]
    for p in range(1, 100):
        if i_sec[p % len(i_sec)] == i_sec[(p + 1) % len(i_sec)] and all(q_sec(q)[p] == q_sec(q)[(p + 1) % 100] == i_sec[p % len(i_sec)] for q, _, _ in PRESENT):
            return system, p
    raise AssertionError("no two code periods of one sign")


@pytest.mark.parametrize("sig_id", sorted(CASES))
def test_search_finds_present_prns_and_rejects_an_absent_one(ctx, sig_id):
    band, fs, pilot, iq = CASES[sig_id]
    n = fs // 1000
    system, period = steady_period(band)
    sats = [signals.Satellite(prn=p, doppler_hz=d, code_delay_chips=c, cn0_dbhz=50.0, system=system, carrier_phase_rad=0.5 + p)
            for p, d, c in PRESENT]
    sig = signals.generate_if(float(fs), n, sats, seed=SEED, start=(period + 1) * n)  # delayed codes: periods `period` and `period` + 1
    prns = [p for p, _, _ in PRESENT] + [ABSENT]
    gen = codes.galileo_e5a_acquisition_code if band == "a" else codes.galileo_e5b_acquisition_code
    sampled = codes.galileo_e5_a_code_gen_complex_sampled if band == "a" else codes.galileo_e5_b_code_gen_complex_sampled
    make = engine.galileo_e5a_pcps_acquisition if band == "a" else engine.galileo_e5b_pcps_acquisition
    acq = make(ctx, fs, 2000, 250, acquire_pilot=pilot, acquire_iq=iq, max_prns=len(prns))
    assert acq.n_bins == 16 and acq.conf.fft_size == n
    assert acq.acquire_iq == iq and acq.acquire_pilot == (pilot and not iq)
    local = {p: gen(p, fs, 1, acq.acquire_pilot, acq.acquire_iq) for p in prns}
    for p in prns:  # the adapter's choice of code: the sampled sig_id code, one period
        assert np.array_equal(local[p], sampled(p, sig_id, fs, 0)) and len(local[p]) == n
        assert np.all(local[p].imag != 0) == (sig_id[1] == "X")
    for i, p in enumerate(prns):
        acq.set_local_code(local[p], i)
    res, _ = acq.run(sig, n_prns=len(prns))
    spc, spcode = acq.conf.samples_per_chip, acq.conf.samples_per_code
    acq.close()
    stats = {}
    for i, p in enumerate(prns):
        ref, rgrid = O.pcps_acquisition_core(sig, local[p], fs, 2000, 250, 0, True, samples_per_chip=spc, samples_per_code=spcode)
        stats[p] = (res[i].test_statistic, ref.test_statistic)
        if p != ABSENT:
            flat = np.sort(rgrid.ravel())
            print(sig_id, p, "margin", flat[-1] / flat[-2], "statistic", res[i].test_statistic, ref.test_statistic)
            assert flat[-1] / flat[-2] > TIE, (p, flat[-1] / flat[-2])
            assert (res[i].doppler_index, res[i].code_index) == (ref.doppler_index, ref.code_index), p
            assert res[i].acq_delay_samples == ref.acq_delay_samples and res[i].doppler_hz == ref.doppler_hz, p
            d, c = next((d, c) for q, d, c in PRESENT if q == p)
            assert abs(res[i].doppler_hz - d) <= 250
            want = (c / 10.23e6 * fs) % n
            assert min(abs(res[i].code_index - want), n - abs(res[i].code_index - want)) <= 2
        np.testing.assert_allclose(res[i].test_statistic, ref.test_statistic, rtol=2e-3)
    # the noise-only CFAR statistic ≈ 2·ln(cells) ≈ 24-27; every present PRN stands above it — a single component
    # carries half the signal's power, and PRN 9's −1210 Hz falls between two bins at 1.22 samples per chip
    assert stats[ABSENT][0] < 30
    assert min(stats[p][0] for p, _, _ in PRESENT) > 1.3 * stats[ABSENT][0]
