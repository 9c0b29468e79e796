"""The BeiDou B3I and GPS L2C scenarios of tests/test_gpu_trk_b3i.py and tests/test_gpu_trk_l2c.py lock in
the oracle loop alone (CPU), configured with the two signals' constants (tests/b3i_l2c_scenarios.py), so a
device mismatch there is the device's.  The ranges stand around figures measured with the oracle."""
import numpy as np
import pytest

from oracle import trk as T

import b3i_l2c_scenarios as B


def first_state_4(ref):
    assert np.any(ref["state"] == 4)
    return int(np.argmax(ref["state"] == 4))


@pytest.mark.parametrize("fs,avx", [(12.5e6, 0), (12.5e6, 1), (8.184e6, 0), (8.184e6, 1)])
def test_b3i_meo_reaches_state_4(fs, avx):
    """C/N0 50 dB-Hz, Doppler +15 Hz off, 120 epochs: state 4 first at epoch 39 (the 20-symbol NH20 search
    after the pull-in); final C/N0 48.5 dB-Hz at 12.5 Msps, 39.4 at 8.184 Msps (which undersamples the code)."""
    epochs = 120
    sat, k, x, stamp, first, delay, dop = B.b3i_sync(fs, epochs, rotator_avx=avx)
    assert k.vector_length == int(round(fs * 1e-3))
    ref = T.track(k, x, sat.code, delay, dop, stamp, first, epochs, buffer_first=first)
    print("B3I", fs, avx, first_state_4(ref), ref["cn0_db_hz"][-1], ref["carrier_doppler_hz"][-1])
    assert len(ref) == epochs and ref["state"][-1] == 4 and np.all(ref["state"] != 0)  # no loss of lock
    assert 20 <= first_state_4(ref) <= 60
    if fs > 10.23e6:
        assert abs(ref["cn0_db_hz"][-1] - 50.0) < 3.0
    else:
        assert ref["cn0_db_hz"][-1] > 35.0


def test_b3i_geo_synchronises_on_the_d2_preamble():
    """GEO PRN 3: 2 code periods per bit, no NH code, the 22-symbol preamble; state 4 first at epoch 41."""
    epochs = 160
    sat, k, x, stamp, first, delay, dop = B.b3i_sync(12.5e6, epochs, prn=3, rotator_avx=1)
    assert k.symbols_per_bit == 2 and k.secondary == 0 and k.secondary_code_length == 22
    ref = T.track(k, x, sat.code, delay, dop, stamp, first, epochs, buffer_first=first)
    print("B3I GEO", first_state_4(ref), ref["cn0_db_hz"][-1])
    assert len(ref) == epochs and ref["state"][-1] == 4
    assert 22 <= first_state_4(ref) <= 70


@pytest.mark.parametrize("fs,avx", [(1.25e6, 0), (1.25e6, 1), (2e6, 1)])
def test_l2c_locks_from_the_first_epoch(fs, avx):
    """C/N0 45 dB-Hz, Doppler +3 Hz off, 60 epochs of 20 ms with the reference's L2C loop bandwidths
    (pll 2 Hz, dll 0.25 Hz): state 4 from epoch 1 (no secondary code, one symbol per bit).  Final C/N0 45.3
    dB-Hz and carrier lock test 0.998 at 1.25 Msps; 43.4 dB-Hz and 0.77 (still converging) at 2 Msps."""
    epochs = 60
    sat, k, x, stamp, first, delay, dop = B.l2c_sync(fs, epochs, rotator_avx=avx)
    assert k.vector_length == int(round(fs / 50)) and k.pll_bw_hz == 2.0 and k.dll_bw_hz == 0.25
    ref = T.track(k, x, sat.code, delay, dop, stamp, first, epochs, buffer_first=first)
    print("L2C", fs, avx, first_state_4(ref), ref["cn0_db_hz"][-1], ref["carrier_lock_test"][-1], ref["carrier_doppler_hz"][-1])
    assert len(ref) == epochs and np.all(ref["state"][1:] == 4)  # state 4 from epoch 1, no loss of lock
    assert abs(ref["carrier_doppler_hz"][-1] - 1210.0) < 5.0
    assert abs(ref["cn0_db_hz"][-1] - 45.0) < 3.0
    assert ref["carrier_lock_test"][-1] > (0.9 if fs == 1.25e6 else 0.6)
