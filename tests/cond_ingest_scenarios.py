"""The packed real-IF scenario of the conditioner-ingest tests: a 16 Msps real-sampled stream, 0.3 s, holding
GPS L1 C/A PRN 7 (1730 Hz, 315.6 chips) and PRN 19 (−2270 Hz, 801.3 chips) at IF +4 MHz with C/N0 50 dB-Hz,
r = √2·Re{generate_if(..., seed=0x2b)}, quantised to 2 bits with thresholds at 0 and ±σ (values ±1, ±3; σ = √2,
the noise's standard deviation in r) and packed four samples to a byte as Two_Bit_Packed_File_Signal_Source
reads them (sample_type real, LSB first) — the layout of conf/gnss-sdr_GPS_L1_nsr_twobit_packed.conf:35-91 at a
small rate.  Conditioned with D = 4 and the adapter's default low-pass taps to 4 Msps, it is the GPS band of
tests/cond_scenarios.py from there on (dwell, acquisition, tracking, truth).  Shared by the CPU companion (model
conditioner + oracle) and the GPU tests (device conditioner, receiver tool)."""
import numpy as np

from gnss_sim_receiver_amd import abi, signals

import cond_ingest_model as I
import cond_model as M
import cond_scenarios as C
import trk_scenarios as S

FS = C.FS
N_IN = C.N_IN
SYSTEM = "GPS"
IF_HZ = C.BANDS[SYSTEM]["if_hz"]
DECIM = C.BANDS[SYSTEM]["decim"]
CN0 = 50.0
SIGMA = float(np.sqrt(2.0))
FMT = abi.fmt_two_bit_packed("real", False)
N_BYTES = N_IN // 4

assert (FS, N_IN, IF_HZ, DECIM) == (16_000_000, 4_800_000, 4_000_000, 4)
assert C.BANDS[SYSTEM]["sats"] == [(7, 1730.0, 315.6), (19, -2270.0, 801.3)]

_CACHE = {}


def satellites():
    return [signals.Satellite(prn=p, doppler_hz=d, code_delay_chips=c, cn0_dbhz=CN0, system=SYSTEM, carrier_phase_rad=0.3 + 0.1 * p,
                              f_if_hz=float(IF_HZ), **S.SYNC_PATTERNS[SYSTEM]) for p, d, c in C.BANDS[SYSTEM]["sats"]]


def packed_stream():
    """(packed bytes uint8[N_IN / 4], the same samples as complex64 exactly as the load converts them)."""
    if "raw" not in _CACHE:
        x = signals.generate_if(float(FS), N_IN, satellites(), seed=0x2b)
        r = np.sqrt(2.0) * x.real.astype(np.float64)
        raw = I.pack(I.quantise_2bit(r, SIGMA), FMT)
        _CACHE["raw"] = (raw, I.unpack(raw, FMT))
    return _CACHE["raw"]


def taps(lib_taps):
    """The adapter's default low-pass taps; lib_taps(fs, decimation) designs them."""
    return lib_taps(float(FS), DECIM)


def model_conditioned(h):
    """The stream as the float64 model conditions it, rounded to complex64."""
    if "model" not in _CACHE:
        _CACHE["model"] = M.model_mix_fir(packed_stream()[1], h, DECIM, IF_HZ, FS).astype(np.complex64)
    return _CACHE["model"]
