"""Galileo E5a / E5b tracking scenarios shared by the oracle (CPU) and device (GPU) tests.

The oracle is parametric in the signal constants (oracle/trk_oracle.c), so its configuration for either
signal is the "GPS" one with every constant overridden (dll_pll_veml_tracking.cc:292-353, start_tracking
:699-746); slope, spc and y_intercept are the values the block — and the engine — derive
(1, early_late_space_chips, 1).

  pilot mode (track_pilot = 1): the tracking code is the Q primary, the data code the I primary; the
      synchronisation pattern is the satellite's own 100-chip secondary code, the I secondary code (20 / 4
      chips) is stripped from the data prompt;
  data-only mode (track_pilot = 0): the tracking code is the I primary; the I secondary code is the
      synchronisation pattern, and d_data_secondary_code_length stays 0.

The oracle has no d_interchange_iq: exchanged() swaps prompt_i / prompt_q in the records whose flag 1
(valid symbol) is set, which is what the block hands to telemetry with the pilot tracked (:1945-1949,
:1997-2001).  State 2's diagnostic prompt and the dump records are not exchanged.

Timing as b3i_l2c_scenarios.b3i_sync (acquisition stamped at sample 0, pull_in_time_s = 0, the delay handed
over 0.2 samples off, Doppler +15 Hz off), except that tracking starts ten code periods before one second:
the first epoch is code period 990, so the 100-entry sign buffer fills with periods 990..1089 and holds the
whole secondary code, periods 1000..1099, ten epochs later — the loops have those ten epochs to settle
before the first sign that has to be right.
"""
import numpy as np

from gnss_sim_receiver_amd import codes, signals
from oracle import trk as T

PERIOD_S = 1e-3
LEAD_PERIODS = 10
BITS = "0110100"  # cyclic I-component symbols of the synthetic signal (20 / 4 code periods each)
BAND = {
    # system of signals.py, carrier, I secondary code, pilot secondary code of a PRN
    "a": ("GAL_E5A", 1176.45e6, codes.GALILEO_E5A_I_SECONDARY_CODE, codes.galileo_e5a_q_secondary),
    "b": ("GAL_E5B", 1207.14e6, codes.GALILEO_E5B_I_SECONDARY_CODE, codes.galileo_e5b_q_secondary),
}
# 260 epochs hold the synchronisation (epoch 110 in pilot mode) and, at E5b's 4 code periods per symbol, more than
# 20 symbols.  E5a has 20 code periods per symbol: 20 symbols after epoch 110 need 510 epochs, so its scenarios run 530.
EPOCHS = {"a": 530, "b": 260}


def conf(band, fs, prn, pilot=True, **kw):
    """The oracle's E5a / E5b configuration at sample rate fs for satellite prn."""
    _, fc, i_sec, q_sec = BAND[band]
    els = kw.get("early_late_space_chips", 0.25)
    base = dict(code_chip_rate=10.23e6, signal_carrier_freq=fc, code_period=PERIOD_S, code_length_chips=10230, code_samples_per_chip=1,
                symbols_per_bit=len(i_sec), secondary=1, pull_in_time_s=0, slope=1.0, spc=els, y_intercept=1.0)
    if pilot:
        sec = q_sec(prn)
        base.update(track_pilot=1, secondary_code=sec.encode(), secondary_code_length=len(sec), data_secondary_code=i_sec.encode(),
                    data_secondary_code_length=len(i_sec))
    else:
        base.update(track_pilot=0, secondary_code=i_sec.encode(), secondary_code_length=len(i_sec), data_secondary_code=b"",
                    data_secondary_code_length=0)
    base.update(kw)
    k = T.conf("GPS", fs, int(round(fs * PERIOD_S)), **base)
    # the adapters' limits (galileo_e5a_dll_pll_tracking.cc:47-58): at least 1; data-only: at most the I secondary length
    k.extend_correlation_symbols = max(k.extend_correlation_symbols, 1)
    if not pilot:
        k.extend_correlation_symbols = min(k.extend_correlation_symbols, len(i_sec))
    return k


def acq_delay_for(sat, fs, stamp, first):
    m = np.ceil(sat.chip_phase(np.float64(first), fs) / sat.code_len)
    n0 = (m * sat.code_len + sat.code_delay_chips) * fs / sat.code_freq()
    return (first - stamp) + np.mod(n0 - first, PERIOD_S * fs)


def satellite(band, prn=11, dop=1210.0, delay_chips=100.3, cn0=50.0, phase=1.0):
    return signals.Satellite(prn=prn, doppler_hz=dop, code_delay_chips=delay_chips, cn0_dbhz=cn0, system=BAND[band][0], carrier_phase_rad=phase,
                             bits=BITS)


def replicas(sat, pilot):
    """(tracking code, data code or None) of a channel on this satellite."""
    return (sat.code, sat.code_data) if pilot else (sat.code_data, None)


def first_sample(fs):
    return int(fs) - LEAD_PERIODS * int(round(fs * PERIOD_S))


def sync(band, fs, epochs=None, prn=11, pilot=True, dop=1210.0, delay_chips=100.3, seed=5, cn0=50.0, **conf_kw):
    """One satellite with both components, (d·sec_I·c_I + j·sec_Q[prn]·c_Q)/√2; x[0] is absolute sample `first`."""
    epochs = EPOCHS[band] if epochs is None else epochs
    sat = satellite(band, prn, dop, delay_chips, cn0)
    k = conf(band, fs, prn, pilot, **conf_kw)
    first = first_sample(fs)
    x = signals.generate_if(fs, k.vector_length * (2 + epochs + 3), [sat], seed=seed, start=first)
    return sat, k, x, 0, first, acq_delay_for(sat, fs, 0, first) + 0.2, sat.doppler_hz + 15.0


def exchanged(rec, pilot=True):
    """The oracle's records as the block hands them on with d_interchange_iq set (pilot mode): the valid symbols'
    prompt_i / prompt_q swapped.  A copy; data-only records are returned as they are."""
    out = rec.copy()
    if pilot:
        w = (out["flags"] & 1) != 0
        out["prompt_i"][w], out["prompt_q"][w] = rec["prompt_q"][w], rec["prompt_i"][w]
    return out


def track(sat, k, x, stamp, first, delay, dop, epochs, pilot=True, dump=False, samples=None):
    """The oracle loop on this scenario, records exchanged as the engine's are (dump records as the oracle wrote them)."""
    code, data = replicas(sat, pilot)
    out = T.track(k, x if samples is None else samples, code, delay, dop, stamp, first, epochs, data_code=data, buffer_first=first, dump=dump,
                  prn=sat.prn)
    if dump:
        return exchanged(out[0], pilot), out[1]
    return exchanged(out, pilot)
