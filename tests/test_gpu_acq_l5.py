"""GPS L5I PCPS acquisition (GpsL5iPcpsAcquisition's parameters, engine.gps_l5i_pcps_acquisition) on the
device vs the oracle's acquisition_core restatement: 25 Msps, 25000-sample search, ±2000 Hz in
250 Hz steps (16 bins), the local code the reference's own sampled L5I chips
(tests/golden/gps_l5_codes_ref.npz).  (bin, index) are compared exactly; the seed was chosen on the
CPU so that the oracle's peak / second-largest margin is above 1 + 1e-4 for both present PRNs —
asserted below, so nothing is skipped."""
import os

import numpy as np
import pytest

from gnss_sim_receiver_amd import codes, engine, signals
from oracle import oracle as O

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gps_l5_codes_ref.npz")
FS, N, DMAX, STEP = 25000000, 25000, 2000, 250
SPC = 3  # ceil(fs / 10.23e6), Acq_Conf::SetDerivedParams with the L5I chip rate
TIE = 1.0 + 1e-4
PRESENT = ((3, -1210.0, 4321.7), (29, 640.0, 9001.2))  # (PRN, Doppler, code delay in chips)
ABSENT = 17
SEED = 31


def fixture_code(prn):
    with np.load(GOLDEN) as g:
        bits = np.unpackbits(g[f"sampled_i_{FS}_{prn}"])[:N]
    return (1.0 - 2.0 * bits.astype(np.float32)).astype(np.complex64)  # L5I lies in the real part


def l5_block():
    sats = [signals.Satellite(prn=p, doppler_hz=d, code_delay_chips=c, cn0_dbhz=50.0, system="GPS_L5", carrier_phase_rad=0.5 + p)
            for p, d, c in PRESENT]
    # the block spans code periods 0 and 1 of both satellites: NH10 = 00… holds one sign there (a sign change
    # inside the 1 ms window would split the coherent sum; the reference's answer to that is bit_transition_flag)
    return signals.generate_if(float(FS), N, sats, seed=SEED, start=N)


def test_l5i_search_finds_present_prns_and_rejects_an_absent_one(ctx):
    sig = l5_block()
    prns = [p for p, _, _ in PRESENT] + [ABSENT]
    local = {p: fixture_code(p) for p, _, _ in PRESENT}
    local[ABSENT] = codes.gps_l5i_acquisition_code(ABSENT, FS)
    for p, _, _ in PRESENT:  # the product's generator gives the fixture's code
        assert np.array_equal(codes.gps_l5i_acquisition_code(p, FS), local[p])
    acq = engine.gps_l5i_pcps_acquisition(ctx, FS, DMAX, STEP, max_prns=len(prns))
    assert acq.n_bins == 16 and acq.conf.samples_per_chip == SPC and acq.conf.fft_size == N
    for k, p in enumerate(prns):
        acq.set_local_code(local[p], k)
    res, _ = acq.run(sig, n_prns=len(prns))
    acq.close()
    stats = {}
    for k, p in enumerate(prns):
        ref, rgrid = O.pcps_acquisition_core(sig, local[p], FS, DMAX, STEP, 0, True, samples_per_chip=SPC)
        stats[p] = (res[k].test_statistic, ref.test_statistic)
        if p != ABSENT:
            flat = np.sort(rgrid.ravel())
            assert flat[-1] / flat[-2] > TIE, (p, flat[-1] / flat[-2])
            assert (res[k].doppler_index, res[k].code_index) == (ref.doppler_index, ref.code_index), p
            assert res[k].acq_delay_samples == ref.acq_delay_samples and res[k].doppler_hz == ref.doppler_hz, p
            # the peak sits at the satellite's Doppler bin and code delay
            d, c = next((d, c) for q, d, c in PRESENT if q == p)
            assert abs(res[k].doppler_hz - d) <= STEP / 2
            want = (c / 10.23e6 * FS) % N
            assert min(abs(res[k].code_index - want), N - abs(res[k].code_index - want)) <= 2
        np.testing.assert_allclose(res[k].test_statistic, ref.test_statistic, rtol=2e-3)
    # noise-only CFAR statistic ≈ 2·ln(cells) ≈ 26 for 16 × 25000 cells; the present PRNs stand far above it
    assert stats[ABSENT][0] < 40
    assert min(stats[p][0] for p, _, _ in PRESENT) > 2 * stats[ABSENT][0]
