"""Synthetic GNSS IF generator and truth-aligned correlator job builder.

    x[n] = Σ_k A_k · c_k(n) · d_k(n) · exp(j(2π(f_IF,k + fD_k)·n/fs + φ_k)) + w[n]

* w: complex Gaussian, σ = 1 per component (as signal_generator_c.cc:540-546);
* A_k = sqrt(2·10^(CN0_k/10) / fs), so that C/N0 = A² / (2σ²/fs);
* c_k: the PRN code clocked at chip_rate·(1 + fD/f_carrier) (code Doppler), delayed by τ_k chips;
* d_k: ±1 data bits (GPS 50 bps = 20 code periods per bit), off by default.

Formats: gr_complex = complex64; ibyte = round(8·x) clipped to ±127, int8 interleaved I,Q.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import codes as C
from .abi import JOB_DTYPE, MAX_TAPS

SYSTEMS = {
    # name: (chip_rate, code_len, carrier_hz, code generator)
    "GPS": (C.GPS_L1_CA_CODE_RATE_CPS, C.GPS_L1_CA_CODE_LENGTH_CHIPS, C.GPS_L1_FREQ_HZ, C.gps_l1_ca_code_gen_float),
    "BDS": (C.BEIDOU_B1I_CODE_RATE_CPS, C.BEIDOU_B1I_CODE_LENGTH_CHIPS, C.BEIDOU_B1I_FREQ_HZ, C.beidou_b1i_code_gen_float),
    # Galileo E1 in units of the sinBOC(1,1) replica (2 samples per chip, 8184 per 4 ms code):
    # the tracking code is the E1-C pilot (track_pilot = true), the data code E1-B
    # (dll_pll_veml_tracking.cc:684-697 with galileo_e1_code_gen_sinboc11_float).
    "GAL": (2.0 * C.GALILEO_E1_CODE_CHIP_RATE_CPS, 2 * C.GALILEO_E1_B_CODE_LENGTH_CHIPS, C.GALILEO_E1_FREQ_HZ,
            lambda prn: C.galileo_e1_code_gen_sinboc11_float("1C", prn)),
    # GPS L5: the tracking code is the L5Q pilot, the data code L5I (dll_pll_veml_tracking.cc:670-678)
    "GPS_L5": (C.GPS_L5Q_CODE_RATE_CPS, C.GPS_L5Q_CODE_LENGTH_CHIPS, C.GPS_L5_FREQ_HZ, C.gps_l5q_code_gen_float),
    # BeiDou B3I: one component, NH20 on MEO / IGSO satellites (a GEO satellite: secondary="", symbols_per_bit=2, as B1I)
    "BDS_B3I": (C.BEIDOU_B3I_CODE_RATE_CPS, C.BEIDOU_B3I_CODE_LENGTH_CHIPS, C.BEIDOU_B3I_FREQ_HZ, C.beidou_b3i_code_gen_float),
    # GPS L2C: the L2 CM code alone (no L2 CL), 20 ms per period = one telemetry symbol, no secondary code
    "GPS_L2C": (C.GPS_L2_M_CODE_RATE_CPS, C.GPS_L2_M_CODE_LENGTH_CHIPS, C.GPS_L2_FREQ_HZ, C.gps_l2c_m_code_gen_float),
    # Galileo E5a / E5b: the tracking code is the Q pilot, the data code the I component (dll_pll_veml_tracking.cc:699-746)
    "GAL_E5A": (C.GALILEO_E5A_CODE_CHIP_RATE_CPS, C.GALILEO_E5A_CODE_LENGTH_CHIPS, C.GALILEO_E5A_FREQ_HZ, C.galileo_e5a_q_code_gen_float),
    "GAL_E5B": (C.GALILEO_E5B_CODE_CHIP_RATE_CPS, C.GALILEO_E5B_CODE_LENGTH_CHIPS, C.GALILEO_E5B_FREQ_HZ, C.galileo_e5b_q_code_gen_float),
    # GLONASS L1 / L2 C/A: FDMA — one code for every satellite; the carrier here is channel 0's, a satellite's own
    # is carrier + freq_channel·FDMA_STEP_HZ (Satellite.carrier_hz), and it sits at that offset in the IF
    "GLO_L1": (C.GLONASS_L1_CA_CODE_RATE_CPS, C.GLONASS_L1_CA_CODE_LENGTH_CHIPS, C.GLONASS_L1_CA_FREQ_HZ,
               lambda prn: C.glonass_l1_ca_code_gen_float()),
    "GLO_L2": (C.GLONASS_L2_CA_CODE_RATE_CPS, C.GLONASS_L2_CA_CODE_LENGTH_CHIPS, C.GLONASS_L2_CA_FREQ_HZ,
               lambda prn: C.glonass_l2_ca_code_gen_float()),
}
# FDMA systems: carrier spacing between adjacent frequency channels
FDMA_STEP_HZ = {"GLO_L1": C.DFRQ1_GLO, "GLO_L2": C.DFRQ2_GLO}
DATA_CODES = {"GAL": lambda prn: C.galileo_e1_code_gen_sinboc11_float("1B", prn), "GPS_L5": C.gps_l5i_code_gen_float,
              "GAL_E5A": C.galileo_e5a_i_code_gen_float, "GAL_E5B": C.galileo_e5b_i_code_gen_float}
# secondary codes a system's satellites carry unless the Satellite names its own, as a function of the PRN
# (the Galileo E5 pilots carry one 100-chip code per satellite): (pilot, data component)
DEFAULT_SECONDARY = {"GPS_L5": lambda prn: (C.GPS_L5Q_NH_CODE_STR, C.GPS_L5I_NH_CODE_STR),
                     "BDS_B3I": lambda prn: (C.BEIDOU_B3I_SECONDARY_CODE_STR, None),
                     "GAL_E5A": lambda prn: (C.galileo_e5a_q_secondary(prn), C.GALILEO_E5A_I_SECONDARY_CODE),
                     "GAL_E5B": lambda prn: (C.galileo_e5b_q_secondary(prn), C.GALILEO_E5B_I_SECONDARY_CODE)}
# how the two components combine: Galileo E1 OS (E1B − E1C)/√2 on one phase; GPS L5 (IS-GPS-705) the
# data component in phase and the pilot in quadrature, (I5 + j·Q5)/√2
# — and Galileo E5a / E5b alike, (d·sec_I·c_I + j·sec_Q[prn]·c_Q)/√2
QUADRATURE_PILOT = {"GPS_L5", "GAL_E5A", "GAL_E5B"}
# code periods per data symbol where a data component exists (E1-B: 1; L5I: 10 — 100 sps; E5a-I: 20; E5b-I: 4)
DATA_SYMBOL_PERIODS = {"GAL": 1, "GPS_L5": 10, "GAL_E5A": 20, "GAL_E5B": 4}
# code periods per navigation bit of a single-component signal when not 20 (L2 CM: one 20 ms period per symbol)
BIT_PERIODS = {"GPS_L2C": 1}


@dataclass
class Satellite:
    prn: int
    doppler_hz: float
    code_delay_chips: float
    carrier_phase_rad: float = 0.0
    cn0_dbhz: float = 45.0
    system: str = "GPS"
    data_bits: bool = False
    bit_seed: int = 0
    f_if_hz: float = 0.0
    code: np.ndarray = field(default=None, repr=False)
    code_data: np.ndarray = field(default=None, repr=False)  # E1-B data component (Galileo)
    # cyclic navigation-bit pattern ('0' → +1, '1' → −1): GPS / BDS one bit per 20 code periods,
    # Galileo one E1-B symbol per code period (250 sps)
    bits: str = None
    # cyclic secondary code, one chip per code period: E1-C CS25 on the Galileo pilot, the B1I NH
    # code on the BeiDou signal
    secondary: str = None
    # cyclic secondary code of the data component, one chip per code period (GPS L5: NH10 on L5I)
    secondary_data: str = None
    # line-of-sight dynamics: the Doppler ramps at this rate from doppler_hz at sample 0
    doppler_rate_hz_s: float = 0.0
    # code periods per navigation bit when not the system default (BeiDou GEO D2: 2)
    symbols_per_bit: int = None
    # FDMA frequency channel k (GLONASS, −7…+6): by default the GLONASS_PRN table's value for the PRN.  The
    # satellite's carrier is the system's + k·FDMA_STEP_HZ, and its signal lies k·FDMA_STEP_HZ above f_if_hz
    # (bits with symbols_per_bit=10 give the 10 ms meander half-bits of the GLONASS data)
    freq_channel: int = None

    def __post_init__(self):
        if self.freq_channel is None and self.system in FDMA_STEP_HZ:
            self.freq_channel = C.glonass_freq_channel(self.prn)
        if self.code is None:
            self.code = SYSTEMS[self.system][3](self.prn)
        if self.code_data is None and self.system in DATA_CODES:
            self.code_data = DATA_CODES[self.system](self.prn)
        if self.system in DEFAULT_SECONDARY and (self.secondary is None or self.secondary_data is None):
            pilot, data = DEFAULT_SECONDARY[self.system](self.prn)
            if self.secondary is None:
                self.secondary = pilot
            if self.secondary_data is None:
                self.secondary_data = data

    @property
    def chip_rate(self):
        return SYSTEMS[self.system][0]

    @property
    def code_len(self):
        return SYSTEMS[self.system][1]

    def carrier_hz(self):
        """The satellite's own carrier: the system's, plus the FDMA channel offset."""
        fc = SYSTEMS[self.system][2]
        return fc + self.freq_channel * FDMA_STEP_HZ[self.system] if self.system in FDMA_STEP_HZ else fc

    def if_hz(self):
        """Where the satellite's carrier lies in the IF stream at zero Doppler: f_if_hz, plus the FDMA channel offset."""
        return self.f_if_hz + self.freq_channel * FDMA_STEP_HZ[self.system] if self.system in FDMA_STEP_HZ else self.f_if_hz

    def code_freq(self):
        return self.chip_rate * (1.0 + self.doppler_hz / self.carrier_hz())

    def chip_phase(self, n: np.ndarray, fs: float) -> np.ndarray:
        """Received code phase [chips] at sample n (unwrapped)."""
        ph = n / fs * self.code_freq() - self.code_delay_chips
        if self.doppler_rate_hz_s:
            ph = ph + 0.5 * self.chip_rate * self.doppler_rate_hz_s / self.carrier_hz() * (n / fs) ** 2
        return ph

    def carrier_phase(self, n: np.ndarray, fs: float) -> np.ndarray:
        ph = 2.0 * np.pi * (self.if_hz() + self.doppler_hz) * (n / fs) + self.carrier_phase_rad
        if self.doppler_rate_hz_s:
            ph = ph + np.pi * self.doppler_rate_hz_s * (n / fs) ** 2
        return ph


def generate_if(fs: float, n_samples: int, sats: list, seed: int = 0, noise: bool = True, start: int = 0,
                block: int = 1 << 20) -> np.ndarray:
    """complex64[n_samples] of synthetic IF starting at absolute sample `start`."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.empty(n_samples, np.complex64)
    for b0 in range(0, n_samples, block):
        b1 = min(n_samples, b0 + block)
        n = np.arange(start + b0, start + b1, dtype=np.float64)
        acc = np.zeros(b1 - b0, np.complex128)
        for s in sats:
            amp = np.sqrt(2.0 * 10.0 ** (s.cn0_dbhz / 10.0) / fs)
            ph = s.chip_phase(n, fs)
            chip = np.floor(ph).astype(np.int64)
            c = s.code[np.mod(chip, s.code_len)].astype(np.float64)
            period = np.floor_divide(chip, s.code_len)
            if s.secondary:
                sec = np.array([1.0 if b == "0" else -1.0 for b in s.secondary])
                c = c * sec[np.mod(period, len(sec))]
            data_sign = 1.0
            if s.bits:
                pat = np.array([1.0 if b == "0" else -1.0 for b in s.bits])
                per_bit = s.symbols_per_bit or (DATA_SYMBOL_PERIODS.get(s.system, 1) if s.code_data is not None else BIT_PERIODS.get(s.system, 20))
                data_sign = pat[np.mod(np.floor_divide(period, per_bit), len(pat))]
            if s.code_data is not None and s.system in QUADRATURE_PILOT:  # GPS L5: (d·NH10·c_I + j·NH20·c_Q)/√2
                cd = data_sign * s.code_data[np.mod(chip, s.code_len)].astype(np.float64)
                if s.secondary_data:
                    sec_d = np.array([1.0 if b == "0" else -1.0 for b in s.secondary_data])
                    cd = cd * sec_d[np.mod(period, len(sec_d))]
                c = (cd + 1j * c) / np.sqrt(2.0)
            elif s.code_data is not None:  # Galileo E1 OS: (E1B − E1C)/√2 with sinBOC(1,1) subcarriers
                c = (data_sign * s.code_data[np.mod(chip, s.code_len)].astype(np.float64) - c) / np.sqrt(2.0)
            else:
                c = c * data_sign
            if s.data_bits:
                periods = np.floor_divide(chip, s.code_len)
                bit_idx = np.floor_divide(periods, 20)
                bits = np.where((np.bitwise_xor(bit_idx * 2654435761 + s.bit_seed, 0x5BD1E995) >> 7) & 1, -1.0, 1.0)
                c = c * bits
            acc += amp * c * np.exp(1j * s.carrier_phase(n, fs))
        if noise:
            acc += rng.standard_normal(b1 - b0) + 1j * rng.standard_normal(b1 - b0)
        out[b0:b1] = acc.astype(np.complex64)
    return out


def to_ibyte(x: np.ndarray, scale: float = 8.0) -> np.ndarray:
    """int8 interleaved I,Q: round(scale·x) clipped to ±127 (the C5 ibyte format)."""
    iq = np.empty(2 * len(x), np.float32)
    iq[0::2] = x.real
    iq[1::2] = x.imag
    return np.clip(np.rint(scale * iq), -127, 127).astype(np.int8)


def to_ishort(x: np.ndarray, scale: float = 256.0) -> np.ndarray:
    iq = np.empty(2 * len(x), np.float32)
    iq[0::2] = x.real
    iq[1::2] = x.imag
    return np.clip(np.rint(scale * iq), -32767, 32767).astype(np.int16)


def truth_jobs(sat: Satellite, fs: float, n_epochs: int, vector_length: int, shifts_chips, code_id: int,
               samples_per_chip: int = 1, first_epoch: int = 1) -> np.ndarray:
    """One correlator job per code period, NCO set from the synthetic truth (as a locked DLL/PLL
    would): epoch e starts at the first sample at or after the start of code period e, with
    rem_code = −(fractional chip at that sample) and rem_carr = carrier phase at that sample.
    Argument meaning/units follow dll_pll_veml_tracking::do_correlation_step (:1037-1048)."""
    jobs = np.zeros(n_epochs, JOB_DTYPE)
    L = sat.code_len
    fcode = sat.code_freq()
    for i in range(n_epochs):
        e = first_epoch + i
        # sample where the received code phase crosses e*L chips
        t_start = (e * L + sat.code_delay_chips) / fcode
        s = int(np.ceil(t_start * fs))
        chip = sat.chip_phase(np.float64(s), fs) - e * L
        carr = np.mod(sat.carrier_phase(np.float64(s), fs), 2 * np.pi)
        jobs[i]["sample_offset"] = s
        jobs[i]["n_samples"] = vector_length
        jobs[i]["code_id"] = code_id
        jobs[i]["n_taps"] = len(shifts_chips)
        jobs[i]["rem_carrier_phase_rad"] = np.float32(carr)
        jobs[i]["phase_step_rad"] = np.float32(2 * np.pi * (sat.if_hz() + sat.doppler_hz) / fs)
        jobs[i]["rem_code_phase_chips"] = np.float32(-chip * samples_per_chip)
        jobs[i]["code_phase_step_chips"] = np.float32(fcode / fs * samples_per_chip)
        sh = np.zeros(MAX_TAPS, np.float32)
        sh[: len(shifts_chips)] = np.asarray(shifts_chips, np.float32) * samples_per_chip
        jobs[i]["shifts_chips"] = sh
    return jobs


def random_sky(n_sats: int, seed: int, system: str = "GPS", cn0: float = 45.0, prns=None, dmax: float = 5000.0):
    """Satellites with fD ~ U[±dmax], τ ~ U[0, L), φ ~ U[0, 2π)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    L = SYSTEMS[system][1]
    prns = list(range(1, n_sats + 1)) if prns is None else list(prns)
    return [Satellite(prn=p, doppler_hz=float(rng.uniform(-dmax, dmax)), code_delay_chips=float(rng.uniform(0, L)),
                      carrier_phase_rad=float(rng.uniform(0, 2 * np.pi)), cn0_dbhz=cn0, system=system) for p in prns]


def generate_if_device(fs: float, n_samples: int, sats: list, seed: int = 0, start: int = 0, device: str = "cuda",
                       block: int = 1 << 23, noise: bool = True):
    """generate_if's signal model evaluated on the GPU with torch (bench inputs of many seconds:
    ~100 M samples): returns a complex64 torch tensor on `device`.  Same x[n] as generate_if
    (phases in float64), but the noise comes from torch's generator, so the samples are not
    numpy's; the bench starts its channels from the same truth either way."""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    out = torch.empty(n_samples, dtype=torch.complex64, device=device)
    codes = {}
    for b0 in range(0, n_samples, block):
        b1 = min(n_samples, b0 + block)
        n = torch.arange(start + b0, start + b1, dtype=torch.float64, device=device)
        acc_re = torch.zeros(b1 - b0, dtype=torch.float64, device=device)
        acc_im = torch.zeros_like(acc_re)
        for s in sats:
            key = id(s)
            if key not in codes:
                codes[key] = (torch.as_tensor(np.asarray(s.code, np.float64), device=device),
                              None if s.code_data is None else torch.as_tensor(np.asarray(s.code_data, np.float64), device=device))
            code, code_d = codes[key]
            amp = float(np.sqrt(2.0 * 10.0 ** (s.cn0_dbhz / 10.0) / fs))
            rate, fc = s.chip_rate, s.carrier_hz()
            ph = n / fs * s.code_freq() - s.code_delay_chips
            if s.doppler_rate_hz_s:
                ph = ph + 0.5 * rate * s.doppler_rate_hz_s / fc * (n / fs) ** 2
            chip = torch.floor(ph).to(torch.int64)
            idx = torch.remainder(chip, s.code_len)
            c = code[idx]
            period = torch.div(chip, s.code_len, rounding_mode="floor")
            if s.secondary:
                sec = torch.as_tensor([1.0 if b == "0" else -1.0 for b in s.secondary], dtype=torch.float64, device=device)
                c = c * sec[torch.remainder(period, len(sec))]
            sign = 1.0
            if s.bits:
                pat = torch.as_tensor([1.0 if b == "0" else -1.0 for b in s.bits], dtype=torch.float64, device=device)
                per_bit = s.symbols_per_bit or (DATA_SYMBOL_PERIODS.get(s.system, 1) if code_d is not None else BIT_PERIODS.get(s.system, 20))
                sign = pat[torch.remainder(torch.div(period, per_bit, rounding_mode="floor"), len(pat))]
            cq = None  # the quadrature component (GPS L5: the pilot)
            if code_d is not None and s.system in QUADRATURE_PILOT:
                cd = sign * code_d[idx]
                if s.secondary_data:
                    sec_d = torch.as_tensor([1.0 if b == "0" else -1.0 for b in s.secondary_data], dtype=torch.float64, device=device)
                    cd = cd * sec_d[torch.remainder(period, len(sec_d))]
                c, cq = cd / np.sqrt(2.0), c / np.sqrt(2.0)
            elif code_d is not None:
                c = (sign * code_d[idx] - c) / np.sqrt(2.0)
            else:
                c = c * sign
            cp = 2.0 * np.pi * (s.if_hz() + s.doppler_hz) * (n / fs) + s.carrier_phase_rad
            if s.doppler_rate_hz_s:
                cp = cp + np.pi * s.doppler_rate_hz_s * (n / fs) ** 2
            cos_cp, sin_cp = torch.cos(cp), torch.sin(cp)
            acc_re += amp * c * cos_cp
            acc_im += amp * c * sin_cp
            if cq is not None:  # (c + j·cq)·e^{j·cp}
                acc_re -= amp * cq * sin_cp
                acc_im += amp * cq * cos_cp
        if noise:
            acc_re += torch.randn(b1 - b0, generator=g, dtype=torch.float64, device=device)
            acc_im += torch.randn(b1 - b0, generator=g, dtype=torch.float64, device=device)
        out[b0:b1] = torch.complex(acc_re.to(torch.float32), acc_im.to(torch.float32))
    return out


def acq_delay_samples(sat: Satellite, fs: float, stamp: int, first: int) -> float:
    """Acq_delay_samples as an acquisition stamped at sample `stamp` reports it for a channel whose
    tracking starts at `first`: the first code start at or after `first` (with code Doppler),
    relative to the stamp modulo the nominal code period (pcps_acquisition.cc:693)."""
    m = np.ceil(sat.chip_phase(np.float64(first), fs) / sat.code_len)
    n0 = (m * sat.code_len + sat.code_delay_chips) * fs / sat.code_freq()
    rate, L, _, _ = SYSTEMS[sat.system]
    t_nom = L / rate * fs
    return (first - stamp) + float(np.mod(n0 - first, t_nom))


def c3_sky(cn0: float = 45.0):
    """a 32-PRN all-sky sweep at 25 Msps with 10 PRNs present (seed 0x6E550003);
    which 10 is drawn from the same seed."""
    seed = 0x6E550003
    rng = np.random.Generator(np.random.PCG64(seed))
    prns = sorted(int(p) for p in rng.choice(np.arange(1, 33), 10, replace=False))
    return random_sky(10, seed=seed, cn0=cn0, prns=prns)


def c1_sky(cn0: float = 45.0, extra=()):
    """BASELINE.md / SURVEY §8d C1: GPS PRN 7 at fD = 1730 Hz with its code delayed 1234 samples at
    4 Msps (315.6 chips), GPS navigation bits (the TLM preamble pattern, so bit synchronisation
    completes); `extra`: more satellites (prn, doppler_hz, delay_samples) for multi-channel runs."""
    fs = 4e6
    sats = []
    for prn, fd, delay in ((7, 1730.0, 1234.0),) + tuple(extra):
        s = Satellite(prn=prn, doppler_hz=fd, code_delay_chips=delay * 1.023e6 / fs, carrier_phase_rad=0.7, cn0_dbhz=cn0)
        s.bits = "1000101100110"
        sats.append(s)
    return sats
