"""The dual-band scenario of the signal-conditioner tests: one 16 Msps ibyte stream holding two GPS L1 C/A
satellites at +4 MHz and two BeiDou B1I MEO satellites at −4 MHz (C/N0 47 dB-Hz, 0.3 s), conditioned to
4 Msps (D 4, 193 default low-pass taps, N = 4000) and 8 Msps (D 2, 97 taps, N = 8000) — the layout of
conf/gnss-sdr_BDS_B3I_GPS_L1_CA_ibyte.conf:41-96 (one Freq_Xlating_Fir_Filter per band) at a small rate.
Shared by the CPU companion (model conditioner + oracle) and the GPU tests (device conditioner)."""
import numpy as np

from gnss_sim_receiver_amd import codes, signals
from oracle import oracle as O
from oracle import trk as T

import cond_model as M
import trk_scenarios as S

FS = 16_000_000
SECONDS = 0.3
N_IN = int(FS * SECONDS)
DOPPLER_MAX, DOPPLER_STEP = 5000, 250

# band: IF, decimation, system, satellites (prn, Doppler, code delay in chips)
BANDS = {
    "GPS": dict(if_hz=4_000_000, decim=4, sats=[(7, 1730.0, 315.6), (19, -2270.0, 801.3)]),
    "BDS": dict(if_hz=-4_000_000, decim=2, sats=[(8, 2480.0, 1200.4), (23, -1020.0, 377.7)]),
}

_CACHE = {}


def satellites(system):
    b = BANDS[system]
    return [signals.Satellite(prn=p, doppler_hz=d, code_delay_chips=c, cn0_dbhz=47.0, system=system, carrier_phase_rad=0.3 + 0.1 * p,
                              f_if_hz=float(b["if_hz"]), **S.SYNC_PATTERNS[system]) for p, d, c in b["sats"]]


def raw_stream():
    """(int8 interleaved I/Q, the same samples as complex64)."""
    if "raw" not in _CACHE:
        x = signals.generate_if(float(FS), N_IN, satellites("GPS") + satellites("BDS"), seed=0x16)
        raw = signals.to_ibyte(x)
        _CACHE["raw"] = (raw, raw.astype(np.float32).view(np.complex64))
    return _CACHE["raw"]


def fs_out(system):
    return FS // BANDS[system]["decim"]


def taps(lib_taps, system):
    """The adapter's default low-pass taps for the band; lib_taps(fs, decimation) designs them."""
    return lib_taps(float(FS), BANDS[system]["decim"])


def model_conditioned(system, h):
    """The band as the float64 model conditions it, rounded to complex64."""
    key = ("model", system)
    if key not in _CACHE:
        b = BANDS[system]
        _CACHE[key] = M.model_mix_fir(raw_stream()[1], h, b["decim"], b["if_hz"], FS).astype(np.complex64)
    return _CACHE[key]


def local_code(system, prn):
    fs = fs_out(system)
    return codes.gps_l1_ca_code_gen_complex_sampled(prn, fs) if system == "GPS" else codes.beidou_b1i_code_gen_complex_sampled(prn, fs)


def acq_args(system):
    """PcpsAcquisition keyword arguments of the band (chip rate: samples_per_chip)."""
    return dict(chip_rate=1023000.0 if system == "GPS" else 2046000.0)


def dwell(system):
    """(first sample, length) of the acquisition dwell in the conditioned stream: the second millisecond
    (the filter is warm)."""
    n = fs_out(system) // 1000
    return n, n


def oracle_acquisition(system, prn, y):
    a, n = dwell(system)
    fs = fs_out(system)
    spc = int(np.ceil(np.float32(fs) / np.float32(acq_args(system)["chip_rate"])))
    res, _ = O.pcps_acquisition_core(y[a:a + n], local_code(system, prn), fs, DOPPLER_MAX, DOPPLER_STEP, 0, True, samples_per_chip=spc)
    return res


def truth_code_index(system, sat, n_taps):
    """Where the dwell's correlation peak belongs: the code start in the input stream, delayed by the
    filter's group delay (T − 1)/2 input samples, in decimated samples relative to the dwell, modulo the
    code period — plus the one sample by which the reference's sampled replica leads (its sample i is the
    chip at time (i + 1)·ts: chip index ceil(ts·(i + 1)/tc) − 1, gps_sdr_signal_replica.cc:145-170,
    beidou_b1i_signal_replica.cc:142-167), so an unfiltered signal peaks in [start + 1, start + 2)."""
    d = BANDS[system]["decim"]
    a, n = dwell(system)
    start_in = sat.code_delay_chips / sat.code_freq() * FS + (n_taps - 1) / 2.0
    return float(np.mod(start_in / d + 1.0 - a, n))


def check_acquisition_against_truth(system, sat, res, n_taps):
    a, n = dwell(system)
    assert abs(res.doppler_hz - sat.doppler_hz) <= DOPPLER_STEP, (system, sat.prn, res.doppler_hz)
    err = np.mod(res.code_index - truth_code_index(system, sat, n_taps) + n / 2, n) - n / 2
    assert abs(err) <= 1.0, (system, sat.prn, res.code_index, truth_code_index(system, sat, n_taps))


def trk_conf(system):
    fs = fs_out(system)
    return T.conf(system, float(fs), fs // 1000, rotator_avx=1)


def trk_start(system, res):
    """(acq_delay_samples, acq_doppler_hz, acq_samplestamp, first_sample) from an acquisition of the dwell:
    tracking starts where the dwell ends."""
    a, n = dwell(system)
    return float(res.code_index % n), float(res.doppler_hz), a, a + n


def epochs(system):
    return int(SECONDS * 1000) - 6


def oracle_track(system, sat, y, res):
    delay, dop, stamp, first = trk_start(system, res)
    return T.track(trk_conf(system), y, sat.code, delay, dop, stamp, first, epochs(system), buffer_first=0, prn=sat.prn)
