"""GPS L5 tracking scenarios shared by the oracle (CPU) and device (GPU) tests.

The oracle is parametric in the signal constants (oracle/trk_oracle.c), so its GPS L5 configuration
is the "GPS" one with every L5 constant overridden (dll_pll_veml_tracking.cc:213-237, GPS_L5.h:32-46,
:167-172); slope, spc and y_intercept are the values the block — and the engine — derive (:224-226).
"""
import numpy as np

from gnss_sim_receiver_amd import signals
from oracle import trk as T

NH20 = "00000100110101001110"  # GPS_L5Q_NH_CODE_STR: the pilot's secondary code
NH10 = "0000110101"            # GPS_L5I_NH_CODE_STR: the data component's
CODE_PERIOD_S = 1e-3
DATA_BITS = "0110100"          # cyclic L5I symbols of the synthetic signal (10 code periods each)


def conf(fs, **kw):
    """The oracle's GPS L5 pilot-tracking configuration at sample rate fs."""
    els = kw.get("early_late_space_chips", 0.25)
    base = dict(track_pilot=1, code_chip_rate=10.23e6, signal_carrier_freq=1176.45e6, code_length_chips=10230, symbols_per_bit=10,
                secondary=1, secondary_code=NH20.encode(), secondary_code_length=20, data_secondary_code=NH10.encode(),
                data_secondary_code_length=10, pull_in_time_s=0, slope=1.0, spc=els, y_intercept=1.0)
    base.update(kw)
    return T.conf("GPS", fs, int(round(fs * CODE_PERIOD_S)), **base)


def acq_delay_for(sat, fs, stamp, first):
    """trk_scenarios.acq_delay_for with the L5 code period."""
    m = np.ceil(sat.chip_phase(np.float64(first), fs) / sat.code_len)
    n0 = (m * sat.code_len + sat.code_delay_chips) * fs / sat.code_freq()
    return (first - stamp) + np.mod(n0 - first, CODE_PERIOD_S * fs)


def satellite(prn=9, dop=1210.0, delay_chips=100.3, cn0=50.0, phase=1.0):
    return signals.Satellite(prn=prn, doppler_hz=dop, code_delay_chips=delay_chips, cn0_dbhz=cn0, system="GPS_L5", carrier_phase_rad=phase,
                             bits=DATA_BITS)


def sync(fs, epochs, prn=9, dop=1210.0, delay_chips=100.3, seed=5, cn0=50.0, lead=None, **conf_kw):
    """One L5 satellite (pilot NH20 in quadrature, data NH10 × symbols in phase), acquisition stamped at
    sample 0 and tracking started one second later (trk_scenarios.sync's timing, pull_in_time_s = 0).
    x[0] is absolute sample `first` = fs."""
    sat = satellite(prn, dop, delay_chips, cn0)
    k = conf(fs, **conf_kw)
    first = int(fs)
    lead = k.vector_length * 2 if lead is None else lead
    x = signals.generate_if(fs, lead + k.vector_length * (epochs + 3), [sat], seed=seed, start=first)
    return sat, k, x, 0, first, acq_delay_for(sat, fs, 0, first) + 0.2, sat.doppler_hz + 15.0
