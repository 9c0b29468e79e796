"""The dual-band scenario of tests/test_gpu_cond_dual_band.py (tests/cond_scenarios.py) locks in the
oracle alone (CPU): the float64 model conditioner (tests/cond_model.py) feeds the oracle acquisition and
the oracle tracking loop, so a device mismatch there is the device's.

Measured with the oracle (model-conditioned stream rounded to complex64, 1 ms dwell at the second
millisecond, 250 Hz bins, tracking started where the dwell ends with Dll_Pll_Conf's defaults, 294 epochs):

    band  PRN  acq Doppler  code index (truth)   final Doppler (truth)   final C/N0   states
    GPS    7     1750        1259 (1259.02)        1732.5 ( 1730)          46.4        2 (pull-in) throughout
    GPS   19    -2250        3159 (3158.14)       -2269.4 (-2270)          44.9        2
    BDS    8     2500        4718 (4718.64)        2477.4 ( 2480)          46.8        2
    BDS   23    -1000        1502 (1501.83)       -1019.5 (-1020)          45.8        2

(pull_in_time_s is 10 s, so 0.3 s of signal stays in the pull-in state; no channel loses lock.)"""
import numpy as np
import pytest

from gnss_sim_receiver_amd import abi, engine

import cond_scenarios as C


@pytest.mark.parametrize("system", ["GPS", "BDS"])
def test_dual_band_scenario_locks_in_the_oracle(built, system):
    lib = abi.load()
    h = C.taps(lambda fs, d: engine.cond_lowpass_taps(lib, fs, d), system)
    assert len(h) == (193 if system == "GPS" else 97)
    y = C.model_conditioned(system, h)
    assert len(y) == C.N_IN // C.BANDS[system]["decim"]
    for sat in C.satellites(system):
        res = C.oracle_acquisition(system, sat.prn, y)
        C.check_acquisition_against_truth(system, sat, res, len(h))
        assert res.test_statistic > 40.0
        ref = C.oracle_track(system, sat, y, res)
        print(system, sat.prn, res.doppler_hz, res.code_index, ref["carrier_doppler_hz"][-1], ref["cn0_db_hz"][-1], np.bincount(ref["state"]))
        assert len(ref) == C.epochs(system) and np.all(ref["state"] == 2)       # pull-in throughout, no loss of lock
        assert abs(ref["carrier_doppler_hz"][-1] - sat.doppler_hz) < 10.0
        assert abs(ref["cn0_db_hz"][-1] - 47.0) < 3.5
