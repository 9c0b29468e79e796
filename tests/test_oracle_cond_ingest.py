"""The packed real-IF scenario of tests/test_gpu_cond_ingest_e2e.py (tests/cond_ingest_scenarios.py) locks in
the oracle alone (CPU): the numpy unpacker and the float64 model conditioner (tests/cond_ingest_model.py,
tests/cond_model.py) feed the oracle acquisition and the oracle tracking loop, so a device mismatch there is the
device's.

Measured with the oracle (2-bit real samples at 16 Msps, IF +4 MHz, conditioned with D 4 and the library's 193
default low-pass taps to 4 Msps, rounded to complex64; 1 ms dwell at the second millisecond, 250 Hz bins,
tracking started where the dwell ends with Dll_Pll_Conf's defaults, 294 epochs):

    PRN  acq Doppler  code index (truth)   statistic   final Doppler (truth)   final C/N0   states
     7     1750        1259 (1259.02)        72.6         1730.2 ( 1730)          45.00        2 (pull-in) throughout
    19    -2250        3158 (3158.14)        62.1        -2265.1 (-2270)          45.39        2

The C/N0 estimate sits about 4.5 dB under the nominal 50 dB-Hz: real sampling keeps half the signal power
against the same noise density after the conditioner (3 dB), the 2-bit quantiser at 0 and ±σ loses about 0.55 dB
and the rest is the band edge of the low-pass; the window below is set around the measured values."""
import math

import numpy as np

from gnss_sim_receiver_amd import abi, engine

import cond_ingest_scenarios as P
import cond_scenarios as C

CN0_MEASURED = 45.2   # between the two measured values


def test_packed_stream_is_the_quantised_real_signal(built):
    raw, x = P.packed_stream()
    assert raw.dtype == np.uint8 and len(raw) == P.N_BYTES == 1_200_000 and len(x) == P.N_IN
    assert not x.imag.any() and set(np.unique(x.real).tolist()) == {-3.0, -1.0, 1.0, 3.0}
    # thresholds at ±σ = ±√2 (the noise alone) of a Gaussian whose variance is 2 + 2·0.0125 with the two signals
    # (each √2·Re of amplitude² 2·10⁵/fs = 0.0125): 2·Q(√2/√2.025) = 32.03 % of the samples are ±3; 4.8e6 samples
    # put the estimate within 3·√(0.32·0.68/4.8e6) = 0.0007 of it
    assert abs(np.mean(np.abs(x.real) == 3.0) - math.erfc(math.sqrt(2.0 / 2.025) / math.sqrt(2.0))) < 0.001
    assert abs(np.mean(x.real > 0) - 0.5) < 0.002


def test_packed_real_if_scenario_locks_in_the_oracle(built):
    lib = abi.load()
    h = P.taps(lambda fs, d: engine.cond_lowpass_taps(lib, fs, d))
    assert len(h) == 193
    y = P.model_conditioned(h)
    assert len(y) == P.N_IN // P.DECIM
    for sat in P.satellites():
        res = C.oracle_acquisition(P.SYSTEM, sat.prn, y)
        C.check_acquisition_against_truth(P.SYSTEM, sat, res, len(h))   # one 250 Hz bin, ±1 decimated sample
        ref = C.oracle_track(P.SYSTEM, sat, y, res)
        print(sat.prn, res.doppler_hz, res.code_index, f"{C.truth_code_index(P.SYSTEM, sat, len(h)):.2f}", f"{res.test_statistic:.1f}",
              f"{ref['carrier_doppler_hz'][-1]:.1f}", f"{ref['cn0_db_hz'][-1]:.2f}", np.bincount(ref["state"]))
        assert res.test_statistic > 40.0
        assert len(ref) == C.epochs(P.SYSTEM) == 294 and np.all(ref["state"] == 2)   # pull-in throughout, no loss of lock
        assert abs(ref["carrier_doppler_hz"][-1] - sat.doppler_hz) < 10.0
        assert abs(ref["cn0_db_hz"][-1] - CN0_MEASURED) < 1.0
