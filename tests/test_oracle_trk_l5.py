"""The GPS L5 scenarios of tests/test_gpu_trk_l5.py lock in the oracle loop alone (CPU): the oracle's
generic signal paths (oracle/trk_oracle.c) synchronise the L5Q pilot's NH20 code, strip NH10 from the
L5I prompt and reach state 4, so a device mismatch there is the device's."""
import numpy as np
import pytest

from gnss_sim_receiver_amd import signals
from oracle import trk as T

import l5_scenarios as L5


@pytest.mark.parametrize("fs,kw", [(12.5e6, {}), (12.5e6, dict(rotator_avx=1)), (8.184e6, dict(rotator_avx=1))])
def test_l5_pilot_reaches_state_4(fs, kw):
    epochs = 120
    sat, k, x, stamp, first, delay, dop = L5.sync(fs, epochs, **kw)
    assert k.vector_length == int(round(fs * 1e-3))
    ref = T.track(k, x, sat.code, delay, dop, stamp, first, epochs, data_code=sat.code_data, buffer_first=first)
    assert len(ref) == epochs and ref["state"][-1] == 4
    n4 = int(np.argmax(ref["state"] == 4))
    assert 20 <= n4 <= 60  # the 20-symbol NH20 search after the pull-in, not a lucky start
    # pilot and data share the power: the pilot's C/N0 is 3 dB under the signal's 50 dB-Hz
    assert abs(ref["cn0_db_hz"][-1] - 47.0) < (3.0 if fs > 10.23e6 else 9.0)  # 8.184 Msps undersamples the 10.23 Mcps code


def test_l5_extended_integration_and_quantised_input_lock():
    """extend_correlation_symbols = 5 shows state-3 and state-4 epochs; the CI16 / CI8 quantised IF locks."""
    sat, k, x, stamp, first, delay, dop = L5.sync(12.5e6, 160, rotator_avx=1, extend_correlation_symbols=5)
    ref = T.track(k, x, sat.code, delay, dop, stamp, first, 160, data_code=sat.code_data, buffer_first=first)
    assert np.sum(ref["state"] == 3) >= 3 * 4 and np.sum(ref["state"] == 4) >= 3
    sat, k, x, stamp, first, delay, dop = L5.sync(12.5e6, 120, rotator_avx=1)
    for raw in (signals.to_ishort(x), signals.to_ibyte(x)):
        xq = raw.astype(np.float32).view(np.complex64)
        ref = T.track(k, xq, sat.code, delay, dop, stamp, first, 120, data_code=sat.code_data, buffer_first=first)
        assert len(ref) == 120 and ref["state"][-1] == 4
