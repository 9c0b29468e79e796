"""BeiDou B3I and GPS L2 CM PCPS acquisition (engine.beidou_b3i_pcps_acquisition, engine.gps_l2_m_pcps_acquisition:
the two adapters' parameters) on the device vs the oracle's acquisition_core restatement.

  B3I  12.5 Msps, a 12500-sample search (1 ms), ±2000 Hz in 250 Hz steps (16 bins), samples_per_chip 2
  L2C  2 Msps, a 40000-sample search (one 20 ms code), ±500 Hz in 50 Hz steps (20 bins), samples_per_chip 4,
       samples_per_code = samples_per_ms · 20

The local codes of the present PRNs are the reference's own sampled chips (tests/golden/b3i_l2c_codes_ref.npz).
(bin, index), acq_delay_samples and doppler_hz are compared exactly; the seed was chosen on the CPU so that the
oracle's peak / second-largest margin is above 1 + 1e-4 for every present PRN (measured 1.105 and 1.084 for
B3I, 1.595 and 1.227 for L2C) — asserted below, so nothing is skipped."""
import os

import numpy as np
import pytest

from gnss_sim_receiver_amd import codes, engine, signals
from oracle import oracle as O

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "b3i_l2c_codes_ref.npz")
TIE = 1.0 + 1e-4
ABSENT = 17
SEED = 31
CASES = {
    # fs, N, doppler_max, doppler_step, bins, samples_per_chip, ms_per_code, chip rate, C/N0, (PRN, Doppler, delay in chips)
    "B3I": dict(fs=12500000, n=12500, dmax=2000, step=250, bins=16, spc=2, ms_per_code=1, rate=10.23e6, cn0=50.0, system="BDS_B3I",
                present=((9, -1210.0, 4321.7), (30, 640.0, 9001.2))),
    "L2C": dict(fs=2000000, n=40000, dmax=500, step=50, bins=20, spc=4, ms_per_code=20, rate=0.5115e6, cn0=42.0, system="GPS_L2C",
                present=((9, -210.0, 4321.7), (30, 140.0, 9001.2))),
}


def fixture_code(name, fs, n, prn):
    with np.load(GOLDEN) as g:
        bits = np.unpackbits(g[f"sampled_b3i_{fs}_{prn}_0" if name == "B3I" else f"sampled_l2c_{fs}_{prn}"])[:n]
    v = (1.0 - 2.0 * bits.astype(np.float32)).astype(np.float32)
    return v.astype(np.complex64) if name == "B3I" else (1j * v).astype(np.complex64)  # B3I in the real part, L2 CM in the imaginary


@pytest.mark.parametrize("name", ["B3I", "L2C"])
def test_search_finds_present_prns_and_rejects_an_absent_one(ctx, name):
    k = CASES[name]
    fs, n = k["fs"], k["n"]
    # Acq_Conf::SetDerivedParams in float: samples_per_code = (fs · 0.001F) · ms_per_code
    spcode = float(np.float32(np.float32(np.float32(fs) * np.float32(0.001)) * np.float32(k["ms_per_code"])))
    assert abs(spcode - n) < 0.01
    # no data bits; the block spans code periods 1 and 2 of every satellite, where B3I's NH20 = 00000… holds one sign
    sats = [signals.Satellite(prn=p, doppler_hz=d, code_delay_chips=c, cn0_dbhz=k["cn0"], system=k["system"], carrier_phase_rad=0.5 + p)
            for p, d, c in k["present"]]
    sig = signals.generate_if(float(fs), n, sats, seed=SEED, start=n)
    prns = [p for p, _, _ in k["present"]] + [ABSENT]
    gen = codes.beidou_b3i_acquisition_code if name == "B3I" else codes.gps_l2c_m_acquisition_code
    local = {p: fixture_code(name, fs, n, p) for p, _, _ in k["present"]}
    local[ABSENT] = gen(ABSENT, fs)
    for p, _, _ in k["present"]:  # the product's generator gives the fixture's code
        assert np.array_equal(gen(p, fs), local[p])
    make = engine.beidou_b3i_pcps_acquisition if name == "B3I" else engine.gps_l2_m_pcps_acquisition
    acq = make(ctx, fs, k["dmax"], k["step"], max_prns=len(prns))
    assert acq.n_bins == k["bins"] and acq.conf.samples_per_chip == k["spc"] and acq.conf.fft_size == n
    assert acq.conf.samples_per_code == spcode
    for i, p in enumerate(prns):
        acq.set_local_code(local[p], i)
    res, _ = acq.run(sig, n_prns=len(prns))
    acq.close()
    stats = {}
    for i, p in enumerate(prns):
        ref, rgrid = O.pcps_acquisition_core(sig, local[p], fs, k["dmax"], k["step"], 0, True, samples_per_chip=k["spc"],
                                             samples_per_code=spcode)
        stats[p] = (res[i].test_statistic, ref.test_statistic)
        if p != ABSENT:
            flat = np.sort(rgrid.ravel())
            print(name, p, "margin", flat[-1] / flat[-2], "statistic", res[i].test_statistic, ref.test_statistic)
            assert flat[-1] / flat[-2] > TIE, (p, flat[-1] / flat[-2])
            assert (res[i].doppler_index, res[i].code_index) == (ref.doppler_index, ref.code_index), p
            assert res[i].acq_delay_samples == ref.acq_delay_samples and res[i].doppler_hz == ref.doppler_hz, p
            # the peak sits at the satellite's code delay and within one Doppler bin of its Doppler (B3I's 1 ms sum has a
            # main lobe of ±1000 Hz: the two bins around 640 Hz differ by 0.1 dB, and the noise picks 500 over 750)
            d, c = next((d, c) for q, d, c in k["present"] if q == p)
            assert abs(res[i].doppler_hz - d) <= k["step"]
            want = (c / k["rate"] * fs) % n
            assert min(abs(res[i].code_index - want), n - abs(res[i].code_index - want)) <= 2
        np.testing.assert_allclose(res[i].test_statistic, ref.test_statistic, rtol=2e-3)
    # the noise-only CFAR statistic ≈ 2·ln(cells) ≈ 25-27; the present PRNs stand far above it
    assert stats[ABSENT][0] < 40
    assert min(stats[p][0] for p, _, _ in k["present"]) > 2 * stats[ABSENT][0]
