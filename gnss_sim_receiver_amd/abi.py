"""ctypes binding of the C ABI (include/gnsship.h) exported by ``libgnsship.so``.

The library is built in-tree (``make`` / ``__graft_entry__.build()``) next to this file.  There is
no fallback: if the shared object is missing or does not export the declared symbols, importing
the engine raises — the product path never degrades to a CPU implementation.
"""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)
LIB_PATH = os.path.join(PKG_DIR, "libgnsship.so")
HEADER_PATH = os.path.join(REPO_DIR, "include", "gnsship.h")

OK, E_INVAL, E_NOMEM, E_DEVICE, E_STATE, E_RCCL = 0, -1, -2, -3, -4, -5
FMT_CF32, FMT_CI16, FMT_CI8 = 0, 1, 2
# read by the signal conditioner only: real-sampled IF (the Freq_Xlating_Fir_Filter adapter's float / short / byte)
FMT_RF32, FMT_RI16, FMT_RI8 = 3, 4, 5
# bit-packed items (GNSSHIP_FMT_PACKED): components, field order in a byte, value map
PACKED_REAL, PACKED_IQ, PACKED_QI = 0, 1, 2
PACKED_LSB_FIRST, PACKED_MSB_FIRST = 0, 1
PACKED_MAP_2S1, PACKED_MAP_S = 0, 1


def fmt_packed(bits: int, components: int, order: int, value_map: int) -> int:
    """GNSSHIP_FMT_PACKED(bits, components, order, map): `bits`-wide two's-complement fields s, 8/bits per byte,
    field j at bit offset bits·j (LSB first) or 8 − bits·(j + 1) (MSB first), value 2s + 1 or s; REAL: one field
    per sample, IQ / QI: fields 2m, 2m + 1 are (re, im) / (im, re)."""
    if bits not in (2, 4) or components not in (0, 1, 2) or order not in (0, 1) or value_map not in (0, 1):
        raise ValueError(f"fmt_packed({bits}, {components}, {order}, {value_map})")
    return 0x100 | (bits << 4) | (components << 2) | (order << 1) | value_map


def fmt_is_packed(fmt: int) -> bool:
    return (fmt & ~0xFF) == 0x100


def fmt_packed_fields(fmt: int):
    """(bits, components, order, map) of a packed format value."""
    return (fmt >> 4) & 0xF, (fmt >> 2) & 0x3, (fmt >> 1) & 0x1, fmt & 0x1


_COMPONENTS = {"real": PACKED_REAL, "iq": PACKED_IQ, "qi": PACKED_QI}


def fmt_two_bit_packed(sample_type: str = "real", big_endian_bytes: bool = False) -> int:
    """Two_Bit_Packed_File_Signal_Source with byte items (sample_type, big_endian_bytes; the adapter's defaults)."""
    return fmt_packed(2, _COMPONENTS[sample_type], PACKED_MSB_FIRST if big_endian_bytes else PACKED_LSB_FIRST, PACKED_MAP_2S1)


def fmt_four_bit_cpx(sample_type: str = "iq") -> int:
    """Four_Bit_Cpx_File_Signal_Source (sample_type iq / qi)."""
    if sample_type not in ("iq", "qi"):
        raise ValueError(f"Four_Bit_Cpx sample_type {sample_type!r}")
    return fmt_packed(4, _COMPONENTS[sample_type], PACKED_LSB_FIRST, PACKED_MAP_2S1)


FMT_NSR = fmt_packed(2, PACKED_REAL, PACKED_LSB_FIRST, PACKED_MAP_S)          # Nsr_File_Signal_Source
FMT_TWO_BIT_CPX = fmt_packed(2, PACKED_IQ, PACKED_MSB_FIRST, PACKED_MAP_2S1)  # Two_Bit_Cpx_File_Signal_Source
# every named preset (tests and mirrors use these)
PACKED_PRESETS = {
    **{f"two_bit_packed_{t}_{'msb' if be else 'lsb'}": fmt_two_bit_packed(t, be) for t in ("real", "iq", "qi") for be in (False, True)},
    "nsr": FMT_NSR,
    "two_bit_cpx": FMT_TWO_BIT_CPX,
    "four_bit_cpx_iq": fmt_four_bit_cpx("iq"),
    "four_bit_cpx_qi": fmt_four_bit_cpx("qi"),
}
STAGE_ANCHORS, STAGE_CORRELATE = 1, 2
MAX_TAPS = 8
_ERRNAMES = {E_INVAL: "E_INVAL", E_NOMEM: "E_NOMEM", E_DEVICE: "E_DEVICE", E_STATE: "E_STATE", E_RCCL: "E_RCCL"}
COMM_ID_BYTES = 128

JOB_DTYPE = np.dtype(
    [
        ("sample_offset", "<i8"),
        ("n_samples", "<i4"),
        ("code_id", "<i4"),
        ("n_taps", "<i4"),
        ("flags", "<i4"),
        ("rem_carrier_phase_rad", "<f4"),
        ("phase_step_rad", "<f4"),
        ("phase_rate_step_rad", "<f4"),
        ("rem_code_phase_chips", "<f4"),
        ("code_phase_step_chips", "<f4"),
        ("code_phase_rate_step_chips", "<f4"),
        ("shifts_chips", "<f4", (MAX_TAPS,)),
    ]
)
assert JOB_DTYPE.itemsize == 80


class AcqConf(ctypes.Structure):
    """gnsship_acq_conf — the Acq_Conf fields acquisition_core reads (acq_conf.h:33-81)."""
    _fields_ = [
        ("fs_in", ctypes.c_int64),
        ("fft_size", ctypes.c_int32),
        ("doppler_max", ctypes.c_int32),
        ("doppler_step", ctypes.c_int32),
        ("doppler_center", ctypes.c_int32),
        ("max_dwells", ctypes.c_int32),
        ("use_cfar", ctypes.c_int32),
        ("samples_per_chip", ctypes.c_int32),
        ("samples_per_code", ctypes.c_float),
        ("max_prns", ctypes.c_int32),
        ("consumed_samples", ctypes.c_int32),
        ("bit_transition_flag", ctypes.c_int32),
        ("resampler_ratio", ctypes.c_float),
        ("resampler_latency_samples", ctypes.c_uint32),
    ]


class AcqResult(ctypes.Structure):
    """gnsship_acq_result — what acquisition_core writes (pcps_acquisition.cc:683-696)."""
    _fields_ = [
        ("doppler_index", ctypes.c_uint32),
        ("code_index", ctypes.c_uint32),
        ("doppler_hz", ctypes.c_int32),
        ("peak", ctypes.c_float),
        ("input_power", ctypes.c_float),
        ("test_statistic", ctypes.c_float),
        ("acq_delay_samples", ctypes.c_double),
    ]


class AcqLayout(ctypes.Structure):
    """gnsship_acq_layout — the transform layout a handle chose (gnsship_acq_layout_get)."""
    _fields_ = [
        ("kind", ctypes.c_int32),
        ("P", ctypes.c_int32),
        ("row_len", ctypes.c_int32),
        ("n_passes", ctypes.c_int32),
        ("radix", ctypes.c_int32 * 16),
        ("ct_rows", ctypes.c_int32),
    ]


assert ctypes.sizeof(AcqLayout) == 84

COND_MAX_BANDS, COND_MAX_TAPS = 4, 4096


class CondBand(ctypes.Structure):
    """gnsship_cond_band — one band of the signal conditioner: the Freq_Xlating_Fir_Filter adapter's IF,
    decimation_factor and taps (freq_xlating_fir_filter.cc:60-62,96-105)."""
    _fields_ = [("if_hz", ctypes.c_double), ("decimation", ctypes.c_int), ("taps", ctypes.POINTER(ctypes.c_float)),
                ("n_taps", ctypes.c_int)]


MIT_PULSE_BLANKING, MIT_NOTCH, MIT_NOTCH_LITE = 0, 1, 2
MIT_CHAIN_AUTO, MIT_CHAIN_SERIAL, MIT_CHAIN_SPECULATIVE = 0, 1, 2
MIT_MAX_LENGTH = 1024


class MitConf(ctypes.Structure):
    """gnsship_mit_conf — the arguments of make_pulse_blanking_cc / make_notch_filter / make_notch_filter_lite
    (pulse_blanking_cc.cc:26, notch_cc.cc:25, notch_lite_cc.cc:26) and the device form of the notch recursion."""
    _fields_ = [("kind", ctypes.c_int32), ("pfa", ctypes.c_float), ("threshold", ctypes.c_float), ("p_c_factor", ctypes.c_float),
                ("length", ctypes.c_int32), ("n_segments_est", ctypes.c_int32), ("n_segments_reset", ctypes.c_int32),
                ("n_segments_coeff", ctypes.c_int32), ("chain_form", ctypes.c_int32)]


class MitState(ctypes.Structure):
    """gnsship_mit_state — the block's members and the chain counters."""
    _fields_ = [("noise_power", ctypes.c_float), ("threshold", ctypes.c_float), ("n_segments", ctypes.c_int32),
                ("n_segments_coeff", ctypes.c_int32), ("filter_state", ctypes.c_int32), ("chain_form", ctypes.c_int32),
                ("samples_in", ctypes.c_uint64), ("samples_out", ctypes.c_uint64), ("pending_samples", ctypes.c_int64),
                ("chunk_samples", ctypes.c_int64), ("warmup_samples", ctypes.c_int64), ("chunks_speculated", ctypes.c_uint64),
                ("chunks_replayed", ctypes.c_uint64)]


VIT_MODE_REFERENCE, VIT_MODE_FULL = 0, 1
VIT_MAX_FRAME_SYMBOLS = 1024


class VitConf(ctypes.Structure):
    """gnsship_vit_conf — Viterbi_Decoder(KK, nn, LL, g) (viterbi_decoder.cc:21-44), the page's interleaver
    (galileo_telemetry_decoder_gs.cc:342-351), the G2 flip (:362-368) and the decoding mode."""
    _fields_ = [("constraint_length", ctypes.c_int32), ("rate_n", ctypes.c_int32), ("g", ctypes.c_int32 * 2),
                ("data_length", ctypes.c_int32), ("interleaver_rows", ctypes.c_int32), ("interleaver_cols", ctypes.c_int32),
                ("invert_g2", ctypes.c_int32), ("mode", ctypes.c_int32)]


TLM_INAV, TLM_FNAV, TLM_CNAV = 1, 2, 3
# gnsship_tlm_page.flags
TLM_CRC_OK, TLM_CRC_EVALUATED, TLM_PLL_180, TLM_ODD, TLM_FRAME_SYNC, TLM_SYNC_LOST = 1, 2, 4, 8, 16, 32
# (preamble length, period, required symbols, data length LL) of the three frame types
TLM_GEOMETRY = {TLM_INAV: (10, 250, 510, 114), TLM_FNAV: (12, 500, 512, 238), TLM_CNAV: (16, 1000, 1016, 486)}


class TlmConf(ctypes.Structure):
    """gnsship_tlm_conf — the frame type of galileo_telemetry_decoder_gs (:167-213), the Viterbi mode and the most
    symbols per channel one run may carry."""
    _fields_ = [("frame_type", ctypes.c_int32), ("vit_mode", ctypes.c_int32), ("max_rounds", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class TlmState(ctypes.Structure):
    """gnsship_tlm_state — the block's members of one channel."""
    _fields_ = [("symbol_counter", ctypes.c_uint64), ("preamble_index", ctypes.c_uint64), ("last_valid_preamble", ctypes.c_uint64),
                ("stat", ctypes.c_int32), ("crc_error_counter", ctypes.c_int32), ("history_size", ctypes.c_int32),
                ("pll_180", ctypes.c_uint8), ("frame_sync", ctypes.c_uint8), ("even_word_arrived", ctypes.c_uint8),
                ("flag_crc_test", ctypes.c_uint8), ("sent_tlm_failed", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 3)]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "pad"}


assert ctypes.sizeof(TlmState) == 48

TLM_PAGE_DTYPE = np.dtype([("symbol_counter", "<u8"), ("sample_counter", "<u8"), ("channel", "<i4"), ("flags", "<i4"),
                           ("crc_error_counter", "<i4"), ("pad", "<i4")])
assert TLM_PAGE_DTYPE.itemsize == 32

# gnsship_lnav_subframe.flags
LNAV_OK, LNAV_PARITY_OK, LNAV_PLL_180, LNAV_STATE1, LNAV_FRAME_SYNC, LNAV_SYNC_LOST = 1, 2, 4, 8, 16, 32
# sflags of an entry (GNSSHIP_LNAV_S_*)
LNAV_S_OUTPUT, LNAV_S_PLL_180, LNAV_S_SUBFRAME = 1, 2, 4


def lnav_subframes_per_run(max_rounds: int) -> int:
    """GNSSHIP_LNAV_SUBFRAMES_PER_RUN."""
    return max_rounds // 300 + max_rounds // 900 + 2


class LnavConf(ctypes.Structure):
    """gnsship_lnav_conf — the most entries per channel one run may carry."""
    _fields_ = [("max_rounds", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class LnavState(ctypes.Structure):
    """gnsship_lnav_state — the members of one channel's gps_l1_ca_telemetry_decoder_gs object."""
    _fields_ = [("symbol_counter", ctypes.c_uint64), ("preamble_index", ctypes.c_uint64), ("last_valid_preamble", ctypes.c_uint64),
                ("subframes_tried", ctypes.c_uint64), ("prev_word", ctypes.c_uint32), ("tow_at_preamble_ms", ctypes.c_uint32),
                ("tow_at_current_symbol_ms", ctypes.c_uint32), ("nav_tow_s", ctypes.c_uint32), ("stat", ctypes.c_int32),
                ("crc_error_counter", ctypes.c_int32), ("history_size", ctypes.c_int32), ("pll_180", ctypes.c_uint8),
                ("frame_sync", ctypes.c_uint8), ("tow_set", ctypes.c_uint8), ("sent_tlm_failed", ctypes.c_uint8)]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


assert ctypes.sizeof(LnavState) == 64

LNAV_SUBFRAME_DTYPE = np.dtype([("symbol_counter", "<u8"), ("sample_counter", "<u8"), ("words", "<u4", (10,)), ("channel", "<i4"),
                                ("subframe_id", "<i4"), ("tow_s", "<u4"), ("crc_error_counter", "<i4"), ("parity_fail_mask", "<u4"),
                                ("flags", "<i4")])
assert LNAV_SUBFRAME_DTYPE.itemsize == 80

# gnsship_cnav_conf.signal
CNAV_L2C, CNAV_L5 = 0, 1
# gnsship_cnav_message.flags
CNAV_CRC_OK, CNAV_INVERTED, CNAV_LOCK = 1, 2, 4
# sflags of an entry (GNSSHIP_CNAV_S_*)
CNAV_S_VALID_WORD, CNAV_S_PLL_180, CNAV_S_MESSAGE = 1, 2, 4


def cnav_messages_per_run(max_rounds: int) -> int:
    """GNSSHIP_CNAV_MESSAGES_PER_RUN."""
    return max_rounds // 300 + 4


class CnavConf(ctypes.Structure):
    """gnsship_cnav_conf — the most entries per channel one run may carry, and the signal (CNAV_L2C / CNAV_L5)."""
    _fields_ = [("max_rounds", ctypes.c_int32), ("signal", ctypes.c_int32), ("reserved", ctypes.c_int32)]


CNAV_MESSAGE_DTYPE = np.dtype([("symbol_counter", "<u8"), ("sample_counter", "<u8"), ("channel", "<i4"), ("tow", "<u4"), ("delay", "<u4"),
                               ("prn", "u1"), ("msg_id", "u1"), ("alert", "u1"), ("part", "u1"), ("raw", "u1", (38,)), ("flags", "u1"),
                               ("reserved", "u1")])
assert CNAV_MESSAGE_DTYPE.itemsize == 72

# gnsship_cnav_part / gnsship_cnav_state: every member of one channel's block object, as numpy records so that a state
# read from one handle can be written to another unchanged
CNAV_PART_DTYPE = np.dtype([("metrics", "<u4", (2, 64)), ("decisions", "<u4", (64, 2)), ("symbols", "u1", (128,)), ("decoded", "u1", (64,)),
                            ("n_symbols", "<u4"), ("n_decoded", "<u4"), ("n_crc_fail", "<u4"), ("decisions_index", "<u4"),
                            ("old_is_metrics2", "u1"), ("preamble_seen", "u1"), ("invert", "u1"), ("message_lock", "u1"), ("crc_ok", "u1"),
                            ("init", "u1"), ("reserved", "u1", (2,))])
assert CNAV_PART_DTYPE.itemsize == 1240
CNAV_STATE_DTYPE = np.dtype([("part", CNAV_PART_DTYPE, (2,)), ("symbol_counter", "<u8"), ("last_valid_preamble", "<u8"), ("tow_s", "<f8"),
                             ("tow_ms", "<u4"), ("tow_at_preamble", "<u4"), ("pll_180", "u1"), ("valid_word", "u1"), ("sent_tlm_failed", "u1"),
                             ("reserved", "u1"), ("reserved2", "<u4")])
assert CNAV_STATE_DTYPE.itemsize == 2520

# gnsship_dnav_conf.signal
DNAV_B1I, DNAV_B3I = 0, 1
# gnsship_dnav_subframe.flags
DNAV_INVERTED, DNAV_STATE1, DNAV_NEW_SOW, DNAV_D2_DECODER, DNAV_D2_TIMING, DNAV_TOW_ZEROED = 1, 2, 4, 8, 16, 32
# sflags of an entry (GNSSHIP_DNAV_S_*)
DNAV_S_VALID_WORD, DNAV_S_SUBFRAME, DNAV_S_INVERTED = 1, 2, 4


def dnav_subframes_per_run(max_rounds: int) -> int:
    """GNSSHIP_DNAV_SUBFRAMES_PER_RUN."""
    return max_rounds // 300 + 1


class DnavConf(ctypes.Structure):
    """gnsship_dnav_conf — the most entries per channel one run may carry, and the signal (DNAV_B1I / DNAV_B3I)."""
    _fields_ = [("max_rounds", ctypes.c_int32), ("signal", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class DnavState(ctypes.Structure):
    """gnsship_dnav_state — the members of one channel's beidou_b1i / beidou_b3i_telemetry_decoder_gs object."""
    _fields_ = [("symbol_counter", ctypes.c_uint64), ("preamble_index", ctypes.c_uint64), ("last_valid_preamble", ctypes.c_uint64),
                ("tow_at_preamble_ms", ctypes.c_uint32), ("tow_at_current_symbol_ms", ctypes.c_uint32), ("sow", ctypes.c_uint32),
                ("symbol_duration_ms", ctypes.c_uint32), ("stat", ctypes.c_int32), ("crc_error_counter", ctypes.c_int32),
                ("history_size", ctypes.c_int32), ("prn", ctypes.c_int32), ("sow_set", ctypes.c_uint8), ("frame_sync", ctypes.c_uint8),
                ("valid_word", ctypes.c_uint8), ("new_sow_available", ctypes.c_uint8), ("sent_tlm_failed", ctypes.c_uint8),
                ("d2_decoder", ctypes.c_uint8), ("d2_timing", ctypes.c_uint8), ("reserved", ctypes.c_uint8)]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


assert ctypes.sizeof(DnavState) == 64

DNAV_SUBFRAME_DTYPE = np.dtype([("symbol_counter", "<u8"), ("sample_counter", "<u8"), ("words", "<u4", (10,)), ("channel", "<i4"),
                                ("fra_id", "<i4"), ("pnum", "<i4"), ("sow", "<u4"), ("corrected_mask", "<u4"),
                                ("tow_at_current_symbol_ms", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
assert DNAV_SUBFRAME_DTYPE.itemsize == 88

# gnsship_gnav_conf.signal
GNAV_L1CA, GNAV_L2CA = 0, 1
# gnsship_gnav_string.flags
GNAV_CRC_OK, GNAV_CORRECTED, GNAV_INVERTED, GNAV_NEW_TOW, GNAV_SLOT_UPDATED, GNAV_NEW_EPHEMERIS, GNAV_NEW_UTC_MODEL = 1, 2, 4, 8, 16, 32, 64
# sflags of an entry (GNSSHIP_GNAV_S_*)
GNAV_S_VALID_WORD, GNAV_S_STRING, GNAV_S_INVERTED = 1, 2, 4


def gnav_strings_per_run(max_rounds: int) -> int:
    """GNSSHIP_GNAV_STRINGS_PER_RUN."""
    return max_rounds // 2000 + 1


class GnavConf(ctypes.Structure):
    """gnsship_gnav_conf — the most entries per channel one run may carry, and the signal (GNAV_L1CA / GNAV_L2CA)."""
    _fields_ = [("max_rounds", ctypes.c_int32), ("signal", ctypes.c_int32), ("reserved", ctypes.c_int32)]


GNAV_STRING_DTYPE = np.dtype([("symbol_counter", "<u8"), ("sample_counter", "<u8"), ("tow", "<f8"), ("bits", "<u4", (3,)), ("channel", "<i4"),
                              ("prn", "<i4"), ("string_id", "<i4"), ("flipped_bit", "<i4"), ("tow_at_current_symbol_ms", "<u4"),
                              ("flags", "<u4"), ("reserved", "<u4")])
assert GNAV_STRING_DTYPE.itemsize == 64
# gnsship_gnav_state — the members of one channel's glonass_l1_ca / glonass_l2_ca_telemetry_decoder_gs object and of its
# navigation object, the string in flight and the history's sign bits
GNAV_STATE_DTYPE = np.dtype([("symbol_counter", "<u8"), ("preamble_index", "<u8"), ("tow_at_current_symbol", "<f8"), ("tow", "<f8"),
                             ("tau_c", "<f8"), ("tau_gps", "<f8"), ("chip_acc", "<f8"), ("stat", "<i4"), ("crc_error_counter", "<i4"),
                             ("history_size", "<i4"), ("prn", "<i4"), ("wn", "<i4"), ("t_k", "<u4"), ("t_b", "<u4"), ("previous_tb", "<u4"),
                             ("n_t", "<u4"), ("n", "<u4"), ("n_4", "<u4"), ("frame_sync", "u1"), ("ephemeris_str", "u1", (4,)),
                             ("utc_model_str_5", "u1"), ("tow_set", "u1"), ("tow_new", "u1"), ("reserved", "u1", (4,)),
                             ("half_pos", "<u4", (6,)), ("half_neg", "<u4", (6,)), ("history", "<u4", (64,))])
assert GNAV_STATE_DTYPE.itemsize == 416

SYS_GPS_L1CA, SYS_GAL_E1, SYS_BDS_B1I, SYS_GPS_L5, SYS_BDS_B3I, SYS_GPS_L2C = 0, 1, 2, 3, 4, 5
SYS_GAL_E5A, SYS_GAL_E5B = 6, 7
SYS_GLO_L1CA, SYS_GLO_L2CA = 8, 9  # glonass_l1_ca / glonass_l2_ca_dll_pll_tracking_cc (include/gnsship.h)
# gnsship_trk_last_engine (include/gnsship.h GNSSHIP_TRK_ENGINE_*)
TRK_ENGINE_NONE, TRK_ENGINE_FAST_LATENCY, TRK_ENGINE_FAST_THROUGHPUT, TRK_ENGINE_PERSIST, TRK_ENGINE_ROUNDS, TRK_ENGINE_LANES = 0, 1, 2, 3, 4, 5
TRK_ENGINE_NAMES = {0: "none", 1: "trk_fast_kernel (latency form)", 2: "trk_fast_kernel (throughput form)", 3: "trk_persist_kernel",
                    4: "round-based loop (trk_step_kernel + correlator)", 5: "trk_lane_kernel (throughput form, one 16-lane row per channel)"}
# rotator dot-product variant (include/gnsship.h GNSSHIP_ROTATOR_*, job flag bits GNSSHIP_JOB_*)
ROTATOR_GENERIC, ROTATOR_AVX, ROTATOR_AUTO = 0, 1, -1
JOB_HIGH_DYN, JOB_ROTATOR_AVX, JOB_ROTATOR_TREE = 1, 2, 4


class TrkPlan(ctypes.Structure):
    """gnsship_trk_plan — gnsship_trk_last_plan: the kernel variant and LDS plan the last run's launch function chose."""
    _fields_ = [(n, ctypes.c_int32) for n in ("engine", "format", "n_taps", "data_prompt", "packed", "sring", "rs", "rg", "lds_bytes", "thru",
                                              "long_plan", "avx", "lane_waves")] + [("reserved", ctypes.c_int32 * 3)]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


assert ctypes.sizeof(TrkPlan) == 64


class TrkConf(ctypes.Structure):
    """gnsship_trk_conf — Dll_Pll_Conf (dll_pll_conf.h:33-80), same names/units; defaults as there
    with the gnss_sdr_flags defaults for cn0_samples/cn0_min/max_*lock_fail/carrier_lock_th.  The
    rotator defaults to ROTATOR_AUTO in every binding (include/gnsship.h): the variant volk_gnsssdr
    dispatches on this host.  if_hz (ABI 2): carrier IF fused into the correlator NCO."""
    _fields_ = [
        ("fs_in", ctypes.c_double), ("carrier_lock_th", ctypes.c_double),
        ("pll_bw_hz", ctypes.c_float), ("dll_bw_hz", ctypes.c_float), ("fll_bw_hz", ctypes.c_float),
        ("early_late_space_chips", ctypes.c_float), ("very_early_late_space_chips", ctypes.c_float),
        ("slope", ctypes.c_float), ("spc", ctypes.c_float), ("y_intercept", ctypes.c_float),
        ("cn0_smoother_alpha", ctypes.c_float), ("carrier_lock_test_smoother_alpha", ctypes.c_float),
        ("pull_in_time_s", ctypes.c_uint32), ("bit_synchronization_time_limit_s", ctypes.c_uint32),
        ("vector_length", ctypes.c_uint32),
        ("pll_filter_order", ctypes.c_int32), ("dll_filter_order", ctypes.c_int32),
        ("cn0_samples", ctypes.c_int32), ("cn0_smoother_samples", ctypes.c_int32),
        ("carrier_lock_test_smoother_samples", ctypes.c_int32), ("cn0_min", ctypes.c_int32),
        ("max_code_lock_fail", ctypes.c_int32), ("max_carrier_lock_fail", ctypes.c_int32),
        ("carrier_aiding", ctypes.c_int32), ("track_pilot", ctypes.c_int32), ("system", ctypes.c_int32),
        ("extend_correlation_symbols", ctypes.c_int32), ("pll_bw_narrow_hz", ctypes.c_float), ("dll_bw_narrow_hz", ctypes.c_float),
        ("early_late_space_narrow_chips", ctypes.c_float), ("very_early_late_space_narrow_chips", ctypes.c_float),
        ("enable_fll_pull_in", ctypes.c_int32), ("enable_fll_steady_state", ctypes.c_int32),
        ("high_dyn", ctypes.c_int32), ("smoother_length", ctypes.c_uint32), ("rotator", ctypes.c_int32),
        ("reserved0", ctypes.c_int32), ("if_hz", ctypes.c_double),
    ]

    @classmethod
    def defaults(cls, system: int, fs_in: float, vector_length: int, **kw) -> "TrkConf":
        c = cls(fs_in=fs_in, carrier_lock_th=0.7, pll_bw_hz=35.0, dll_bw_hz=2.0, fll_bw_hz=35.0,
                early_late_space_chips=0.25, very_early_late_space_chips=0.5, slope=1.0, spc=0.5, y_intercept=1.0,
                cn0_smoother_alpha=0.002, carrier_lock_test_smoother_alpha=0.002, pull_in_time_s=10,
                bit_synchronization_time_limit_s=20, vector_length=vector_length, pll_filter_order=3, dll_filter_order=2,
                cn0_samples=20, cn0_smoother_samples=200, carrier_lock_test_smoother_samples=25, cn0_min=25,
                max_code_lock_fail=50, max_carrier_lock_fail=5000, carrier_aiding=1, track_pilot=1, system=system,
                extend_correlation_symbols=1, pll_bw_narrow_hz=5.0, dll_bw_narrow_hz=0.75, early_late_space_narrow_chips=0.15,
                very_early_late_space_narrow_chips=0.5, enable_fll_pull_in=0, enable_fll_steady_state=0,
                high_dyn=0, smoother_length=10, rotator=ROTATOR_AUTO, reserved0=0, if_hz=0.0)
        for k, v in kw.items():
            setattr(c, k, v)
        return c


class TrkStartArgs(ctypes.Structure):
    """gnsship_trk_start_args — the Gnss_Synchro fields start_tracking reads (:647-649)."""
    _fields_ = [("code_id", ctypes.c_int32), ("data_code_id", ctypes.c_int32), ("acq_delay_samples", ctypes.c_double),
                ("acq_doppler_hz", ctypes.c_double), ("acq_samplestamp_samples", ctypes.c_uint64), ("first_sample", ctypes.c_uint64),
                ("prn", ctypes.c_int32), ("reserved", ctypes.c_int32)]


TRK_EPOCH_DTYPE = np.dtype([
    ("sample_counter", "<u8"), ("prompt_i", "<f8"), ("prompt_q", "<f8"), ("code_phase_samples", "<f8"),
    ("carrier_phase_rads", "<f8"), ("carrier_doppler_hz", "<f8"), ("cn0_db_hz", "<f8"), ("carrier_lock_test", "<f4"),
    ("state", "<i4"), ("flags", "<i4"), ("pad", "<i4"), ("code_freq_chips", "<f8"), ("rem_code_phase_chips", "<f8"),
    ("rem_carr_phase_rad", "<f4"), ("prn_length_samples", "<i4"),
])
assert TRK_EPOCH_DTYPE.itemsize == 96

# gnsship_trk_dump_record = the record dll_pll_veml_tracking::log_data writes (:1376-1466), packed
TRK_DUMP_DTYPE = np.dtype([
    ("abs_VE", "<f4"), ("abs_E", "<f4"), ("abs_P", "<f4"), ("abs_L", "<f4"), ("abs_VL", "<f4"), ("prompt_I", "<f4"), ("prompt_Q", "<f4"),
    ("PRN_start_sample_count", "<u8"), ("acc_carrier_phase_rad", "<f4"), ("carrier_doppler_hz", "<f4"), ("carrier_doppler_rate_hz", "<f4"),
    ("code_freq_chips", "<f4"), ("code_freq_rate_chips", "<f4"), ("carr_error_hz", "<f4"), ("carr_error_filt_hz", "<f4"),
    ("code_error_chips", "<f4"), ("code_error_filt_chips", "<f4"), ("CN0_SNV_dB_Hz", "<f4"), ("carrier_lock_test", "<f4"),
    ("aux1", "<f4"), ("aux2", "<f8"), ("PRN", "<u4"),
])
assert TRK_DUMP_DTYPE.itemsize == 96
TRK_FLAG_DUMP = 16
# the record glonass_l1_ca_dll_pll_tracking_cc writes (:641-701): the same without the two rate fields, 88 bytes
TRK_DUMP_GLONASS_DTYPE = np.dtype([(n, TRK_DUMP_DTYPE.fields[n][0]) for n in TRK_DUMP_DTYPE.names
                                   if n not in ("carrier_doppler_rate_hz", "code_freq_rate_chips")])
assert TRK_DUMP_GLONASS_DTYPE.itemsize == 88

# gnsship_trk_corr_trace: one channel-epoch's do_correlation_step arguments and outputs
TRK_TRACE_DTYPE = np.dtype([
    ("sample_counter", "<u8"), ("n_samples", "<i4"), ("n_taps", "<i4"), ("rem_carrier_phase_rad", "<f4"), ("phase_step_rad", "<f4"),
    ("rem_code_phase_samples", "<f4"), ("code_phase_step_samples", "<f4"), ("shifts", "<f4", (5,)), ("taps", "<f4", (10,)),
    ("data_prompt", "<f4", (2,)), ("pad", "<i4"),
])
assert TRK_TRACE_DTYPE.itemsize == 104


class GnssHipError(RuntimeError):
    def __init__(self, code: int, what: str):
        super().__init__(f"{what} failed: {_ERRNAMES.get(code, code)}")
        self.code = code


_vp = ctypes.c_void_p
_vpp = ctypes.POINTER(ctypes.c_void_p)
_f32p = ctypes.POINTER(ctypes.c_float)
_i = ctypes.c_int
_f = ctypes.c_float

_SIGNATURES = {
    "gnsship_abi_version": ([], _i),
    "gnsship_rotator_dispatch": ([ctypes.POINTER(_i)], _i),
    "gnsship_rotator_dispatch_detail": ([ctypes.c_char_p, _i], _i),
    "gnsship_device_count": ([ctypes.POINTER(_i)], _i),
    "gnsship_ctx_create": ([_i, _vpp], _i),
    "gnsship_ctx_destroy": ([_vp], _i),
    "gnsship_last_error": ([_vp], ctypes.c_char_p),
    "gnsship_ctx_sync": ([_vp], _i),
    "gnsship_ctx_stream": ([_vp, _vpp], _i),
    "gnsship_ctx_event_record": ([_vp, _i], _i),
    "gnsship_ctx_event_elapsed_ms": ([_vp, _i, _i, _f32p], _i),
    "gnsship_dev_alloc": ([_vp, ctypes.c_size_t, _vpp], _i),
    "gnsship_dev_free": ([_vp, _vp], _i),
    "gnsship_dev_upload": ([_vp, _vp, _vp, ctypes.c_size_t], _i),
    "gnsship_dev_download": ([_vp, _vp, _vp, ctypes.c_size_t], _i),
    "gnsship_code_set": ([_vp, _i, _f32p, _i], _i),
    "gnsship_code_count": ([_vp, ctypes.POINTER(_i)], _i),
    "gnsship_gps_l1_ca_code_gen_float": ([_f32p, ctypes.c_int32, ctypes.c_uint32], _i),
    "gnsship_gps_l1_ca_code_gen_complex_sampled": ([_f32p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint32], _i),
    "gnsship_beidou_b1i_code_gen_float": ([_f32p, ctypes.c_int32, ctypes.c_uint32], _i),
    "gnsship_beidou_b1i_code_gen_complex_sampled": ([_f32p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint32], _i),
    "gnsship_gps_l5i_code_gen_float": ([_f32p, ctypes.c_int32], _i),
    "gnsship_gps_l5q_code_gen_float": ([_f32p, ctypes.c_int32], _i),
    "gnsship_gps_l5i_code_gen_complex_sampled": ([_f32p, ctypes.c_uint32, ctypes.c_int32], _i),
    "gnsship_gps_l5q_code_gen_complex_sampled": ([_f32p, ctypes.c_uint32, ctypes.c_int32], _i),
    "gnsship_beidou_b3i_code_gen_float": ([_f32p, ctypes.c_int32, ctypes.c_uint32], _i),
    "gnsship_galileo_e5_a_code_gen_complex_primary": ([_f32p, ctypes.c_int32, ctypes.c_char_p], _i),
    "gnsship_galileo_e5_b_code_gen_complex_primary": ([_f32p, ctypes.c_int32, ctypes.c_char_p], _i),
    "gnsship_galileo_e5_a_code_gen_complex_sampled": ([_f32p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_int32, ctypes.c_uint32], _i),
    "gnsship_galileo_e5_b_code_gen_complex_sampled": ([_f32p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_int32, ctypes.c_uint32], _i),
    "gnsship_galileo_e5a_i_code_gen_float": ([_f32p, ctypes.c_int32], _i),
    "gnsship_galileo_e5a_q_code_gen_float": ([_f32p, ctypes.c_int32], _i),
    "gnsship_galileo_e5b_i_code_gen_float": ([_f32p, ctypes.c_int32], _i),
    "gnsship_galileo_e5b_q_code_gen_float": ([_f32p, ctypes.c_int32], _i),
    "gnsship_galileo_e5a_i_secondary_code": ([ctypes.c_char_p], _i),
    "gnsship_galileo_e5b_i_secondary_code": ([ctypes.c_char_p], _i),
    "gnsship_galileo_e5a_q_secondary_code": ([ctypes.c_char_p, ctypes.c_int32], _i),
    "gnsship_galileo_e5b_q_secondary_code": ([ctypes.c_char_p, ctypes.c_int32], _i),
    "gnsship_beidou_b3i_code_gen_complex_sampled": ([_f32p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint32], _i),
    "gnsship_gps_l2c_m_code_gen_float": ([_f32p, ctypes.c_int32], _i),
    "gnsship_gps_l2c_m_code_gen_complex_sampled": ([_f32p, ctypes.c_uint32, ctypes.c_int32], _i),
    "gnsship_glonass_l1_ca_code_gen_float": ([_f32p, ctypes.c_uint32], _i),
    "gnsship_glonass_l1_ca_code_gen_complex": ([_f32p, ctypes.c_uint32], _i),
    "gnsship_glonass_l1_ca_code_gen_complex_sampled": ([_f32p, ctypes.c_int32, ctypes.c_uint32], _i),
    "gnsship_glonass_l2_ca_code_gen_float": ([_f32p, ctypes.c_uint32], _i),
    "gnsship_glonass_l2_ca_code_gen_complex": ([_f32p, ctypes.c_uint32], _i),
    "gnsship_glonass_l2_ca_code_gen_complex_sampled": ([_f32p, ctypes.c_int32, ctypes.c_uint32], _i),
    "gnsship_glonass_freq_channel": ([ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)], _i),
    "gnsship_code_samples_per_code": ([ctypes.c_int32, ctypes.c_int32, ctypes.c_int32], _i),
    "gnsship_corr_create": ([_vp, _i, _i, _vpp], _i),
    "gnsship_corr_set_local_code_and_taps": ([_vp, _i, _f32p, _f32p], _i),
    "gnsship_corr_set_high_dynamics_resampler": ([_vp, _i], _i),
    "gnsship_corr_set_rotator": ([_vp, _i], _i),
    "gnsship_corr_run": ([_vp, _vp, _i, _i, _f, _f, _f, _f, _f, _f, _i, _f32p], _i),
    "gnsship_corr_destroy": ([_vp], _i),
    "gnsship_batch_create": ([_vp, _i, _vpp], _i),
    "gnsship_batch_set_jobs": ([_vp, _vp, _i, ctypes.c_int64], _i),
    "gnsship_batch_launch": ([_vp, _vp, _i], _i),
    "gnsship_batch_launch_stages": ([_vp, _vp, _i, _i], _i),
    "gnsship_batch_results": ([_vp, _f32p], _i),
    "gnsship_batch_results_device": ([_vp, _vpp], _i),
    "gnsship_batch_launch_pipelined": ([_vp, _vp, _i, _vp], _i),
    "gnsship_batch_launch_pipelined2": ([_vp, _vp, _i, _vp, _vp], _i),
    "gnsship_batch_destroy": ([_vp], _i),
    "gnsship_acq_create": ([_vp, ctypes.POINTER(AcqConf), _vpp], _i),
    "gnsship_acq_set_grid": ([_vp, _i, _i, _i], _i),
    "gnsship_acq_set_grid_step2": ([_vp, _f, _f, _i, _f], _i),
    "gnsship_acq_set_local_code": ([_vp, _i, _f32p], _i),
    "gnsship_acq_run": ([_vp, _vp, _i, _i, _i, ctypes.POINTER(AcqResult), _f32p], _i),
    "gnsship_acq_num_bins": ([_vp, ctypes.POINTER(_i)], _i),
    "gnsship_acq_layout_get": ([_vp, ctypes.POINTER(AcqLayout)], _i),
    "gnsship_acq_set_grid_fdma": ([_vp, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_int32)], _i),
    "gnsship_acq_run_fdma": ([_vp, _vp, _i, _i, _i, ctypes.POINTER(AcqResult), _f32p], _i),
    "gnsship_acq_reset_dwells": ([_vp], _i),
    "gnsship_acq_destroy": ([_vp], _i),
    "gnsship_firdes_low_pass": ([ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, _f32p, _i, ctypes.POINTER(_i)], _i),
    "gnsship_acq_resampler_design": ([ctypes.c_int64, ctypes.c_double, ctypes.POINTER(_i), _f32p, _i, ctypes.POINTER(_i)], _i),
    "gnsship_acq_resampler_create": ([_vp, _f32p, _i, _i, ctypes.c_int64, _vpp], _i),
    "gnsship_acq_resampler_run": ([_vp, _vp, _i, _i, ctypes.c_int64, _f32p, _vpp, ctypes.POINTER(ctypes.c_int64)], _i),
    "gnsship_acq_resampler_reset": ([_vp], _i),
    "gnsship_acq_resampler_destroy": ([_vp], _i),
    "gnsship_cond_lowpass_taps": ([ctypes.c_double, _i, ctypes.c_double, ctypes.c_double, _f32p, _i, ctypes.POINTER(_i)], _i),
    "gnsship_cond_fmt_bits": ([_i], _i),
    "gnsship_cond_create": ([_vp, ctypes.c_double, ctypes.POINTER(CondBand), _i, ctypes.c_int64, _vpp], _i),
    "gnsship_cond_run": ([_vp, _vp, _i, _i, ctypes.c_int64, _vpp, ctypes.POINTER(_f32p), _vpp, ctypes.POINTER(ctypes.c_int64)], _i),
    "gnsship_cond_reset": ([_vp, ctypes.c_uint64], _i),
    "gnsship_cond_samples_in": ([_vp, ctypes.POINTER(ctypes.c_uint64)], _i),
    "gnsship_cond_destroy": ([_vp], _i),
    "gnsship_mit_threshold": ([ctypes.c_double, _i, _f32p], _i),
    "gnsship_mit_create": ([_vp, ctypes.POINTER(MitConf), ctypes.c_int64, _vpp], _i),
    "gnsship_mit_run": ([_vp, _vp, _i, ctypes.c_int64, _vp, _f32p, _vpp, ctypes.POINTER(ctypes.c_int64)], _i),
    "gnsship_mit_reset": ([_vp], _i),
    "gnsship_mit_state_get": ([_vp, ctypes.POINTER(MitState)], _i),
    "gnsship_mit_destroy": ([_vp], _i),
    "gnsship_vit_create": ([_vp, ctypes.POINTER(VitConf), ctypes.c_int32, _vpp], _i),
    "gnsship_vit_run": ([_vp, _vp, _i, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8),
                         ctypes.POINTER(ctypes.c_uint8), _vp], _i),
    "gnsship_vit_reset_channel": ([_vp, ctypes.c_int32], _i),
    "gnsship_vit_state_get": ([_vp, ctypes.c_int32, _f32p], _i),
    "gnsship_vit_destroy": ([_vp], _i),
    "gnsship_trk_create": ([_vp, ctypes.POINTER(TrkConf), _i, _vpp], _i),
    "gnsship_trk_start": ([_vp, _i, ctypes.POINTER(TrkStartArgs)], _i),
    "gnsship_trk_start_many": ([_vp, _i, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(TrkStartArgs)], _i),
    "gnsship_trk_stop": ([_vp, _i], _i),
    "gnsship_trk_telemetry_event": ([_vp, _i, _i], _i),
    "gnsship_trk_run": ([_vp, _vp, _i, _i, ctypes.c_uint64, ctypes.c_int64, _i, _vp, ctypes.POINTER(_i)], _i),
    "gnsship_trk_run_dump": ([_vp, _vp, _i, _i, ctypes.c_uint64, ctypes.c_int64, _i, _vp, _vp, ctypes.POINTER(_i)], _i),
    "gnsship_trk_launch": ([_vp, _vp, _i, ctypes.c_uint64, ctypes.c_int64, _i, _i, _i], _i),
    "gnsship_trk_collect": ([_vp, _vp, _vp, ctypes.POINTER(_i)], _i),
    "gnsship_trk_records_device": ([_vp, _vpp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)], _i),
    "gnsship_tlm_create": ([_vp, ctypes.POINTER(TlmConf), ctypes.c_int32, _vpp], _i),
    "gnsship_tlm_run_symbols": ([_vp, _vp, _vp, _i, ctypes.c_int32, _vp, _vp, _vp, _vp], _i),
    "gnsship_tlm_run_records": ([_vp, _vp, _i, ctypes.c_int32, _vp, _vp, _vp, _vp], _i),
    "gnsship_tlm_run_trk": ([_vp, _vp, _vp, _vp, _vp, _vp], _i),
    "gnsship_tlm_outputs_device": ([_vp, _vpp, _vpp, _vpp, _vpp, ctypes.POINTER(ctypes.c_int32)], _i),
    "gnsship_tlm_reset_channel": ([_vp, ctypes.c_int32], _i),
    "gnsship_tlm_set_satellite": ([_vp, ctypes.c_int32], _i),
    "gnsship_tlm_new_channel": ([_vp, ctypes.c_int32], _i),
    "gnsship_tlm_state_get": ([_vp, ctypes.c_int32, ctypes.POINTER(TlmState)], _i),
    "gnsship_tlm_destroy": ([_vp], _i),
    "gnsship_lnav_create": ([_vp, ctypes.POINTER(LnavConf), ctypes.c_int32, _vpp], _i),
    "gnsship_lnav_run_symbols": ([_vp, _vp, _vp, _vp, _i, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp], _i),
    "gnsship_lnav_run_records": ([_vp, _vp, _i, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp], _i),
    "gnsship_lnav_run_trk": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_int32)], _i),
    "gnsship_lnav_outputs_device": ([_vp, _vpp, _vpp, _vpp, _vpp, _vpp, ctypes.POINTER(ctypes.c_int32)], _i),
    "gnsship_lnav_reset_channel": ([_vp, ctypes.c_int32], _i),
    "gnsship_lnav_set_satellite": ([_vp, ctypes.c_int32], _i),
    "gnsship_lnav_new_channel": ([_vp, ctypes.c_int32], _i),
    "gnsship_lnav_state_get": ([_vp, ctypes.c_int32, ctypes.POINTER(LnavState)], _i),
    "gnsship_lnav_destroy": ([_vp], _i),
    "gnsship_cnav_create": ([_vp, ctypes.POINTER(CnavConf), ctypes.c_int32, _vpp], _i),
    "gnsship_cnav_run_symbols": ([_vp, _vp, _vp, _vp, _i, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp], _i),
    "gnsship_cnav_run_records": ([_vp, _vp, _i, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp], _i),
    "gnsship_cnav_run_trk": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_int32)], _i),
    "gnsship_cnav_outputs_device": ([_vp, _vpp, _vpp, _vpp, _vpp, _vpp, ctypes.POINTER(ctypes.c_int32)], _i),
    "gnsship_cnav_reset_channel": ([_vp, ctypes.c_int32], _i),
    "gnsship_cnav_new_channel": ([_vp, ctypes.c_int32], _i),
    "gnsship_cnav_state_get": ([_vp, ctypes.c_int32, _vp], _i),
    "gnsship_cnav_state_set": ([_vp, ctypes.c_int32, _vp], _i),
    "gnsship_cnav_destroy": ([_vp], _i),
    "gnsship_dnav_create": ([_vp, ctypes.POINTER(DnavConf), ctypes.c_int32, _vpp], _i),
    "gnsship_dnav_run_symbols": ([_vp, _vp, _vp, _vp, _i, ctypes.c_int32, _vp, _vp, _vp, _vp], _i),
    "gnsship_dnav_run_records": ([_vp, _vp, _i, ctypes.c_int32, _vp, _vp, _vp, _vp], _i),
    "gnsship_dnav_run_trk": ([_vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_int32)], _i),
    "gnsship_dnav_outputs_device": ([_vp, _vpp, _vpp, _vpp, _vpp, ctypes.POINTER(ctypes.c_int32)], _i),
    "gnsship_dnav_reset_channel": ([_vp, ctypes.c_int32], _i),
    "gnsship_dnav_set_satellite": ([_vp, ctypes.c_int32, ctypes.c_int32], _i),
    "gnsship_dnav_new_channel": ([_vp, ctypes.c_int32, ctypes.c_int32], _i),
    "gnsship_dnav_state_get": ([_vp, ctypes.c_int32, ctypes.POINTER(DnavState)], _i),
    "gnsship_dnav_destroy": ([_vp], _i),
    "gnsship_gnav_create": ([_vp, ctypes.POINTER(GnavConf), ctypes.c_int32, _vpp], _i),
    "gnsship_gnav_run_symbols": ([_vp, _vp, _vp, _vp, _i, ctypes.c_int32, _vp, _vp, _vp, _vp], _i),
    "gnsship_gnav_run_records": ([_vp, _vp, _i, ctypes.c_int32, _vp, _vp, _vp, _vp], _i),
    "gnsship_gnav_run_trk": ([_vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_int32)], _i),
    "gnsship_gnav_outputs_device": ([_vp, _vpp, _vpp, _vpp, _vpp, ctypes.POINTER(ctypes.c_int32)], _i),
    "gnsship_gnav_set_satellite": ([_vp, ctypes.c_int32, ctypes.c_int32], _i),
    "gnsship_gnav_new_channel": ([_vp, ctypes.c_int32, ctypes.c_int32], _i),
    "gnsship_gnav_state_get": ([_vp, ctypes.c_int32, _vp], _i),
    "gnsship_gnav_state_set": ([_vp, ctypes.c_int32, _vp], _i),
    "gnsship_gnav_destroy": ([_vp], _i),
    "gnsship_trk_set_trace": ([_vp, _i], _i),
    "gnsship_trk_trace_records": ([_vp, _vp, _i], _i),
    "gnsship_trk_channel_state": ([_vp, _i, ctypes.POINTER(_i), ctypes.POINTER(ctypes.c_uint64)], _i),
    "gnsship_trk_last_engine": ([_vp, ctypes.POINTER(_i)], _i),
    "gnsship_trk_last_plan": ([_vp, ctypes.POINTER(TrkPlan)], _i),
    "gnsship_trk_destroy": ([_vp], _i),
    "gnsship_comm_unique_id": ([_vp], _i),
    "gnsship_comm_create": ([_vp, _i, _i, _vp, _vpp], _i),
    "gnsship_comm_rank": ([_vp, ctypes.POINTER(_i), ctypes.POINTER(_i)], _i),
    "gnsship_comm_broadcast": ([_vp, _vp, ctypes.c_size_t, _i], _i),
    "gnsship_comm_allgather": ([_vp, _vp, _vp, ctypes.c_size_t], _i),
    "gnsship_comm_allreduce_max_f64": ([_vp, _vp, ctypes.c_size_t], _i),
    "gnsship_comm_destroy": ([_vp], _i),
}


def declared_symbols(header: str = HEADER_PATH) -> list:
    """Every function name declared in include/gnsship.h."""
    text = open(header).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gnsship_[a-z0-9_]+)\s*\(", text)))


_LIB = None


ABI_VERSION = 2  # GNSSHIP_ABI_VERSION of the header these bindings mirror


def load() -> ctypes.CDLL:
    """Load libgnsship.so (raises if it was not built — no fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # GNSSHIP_LIB_PATH: tooling only (scripts/corr_wg_profile.py loads the instrumented build)
    path = os.environ.get("GNSSHIP_LIB_PATH", LIB_PATH)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `make` or __graft_entry__.build(); "
                           "the GNSS engine has no CPU fallback")
    lib = ctypes.CDLL(path)
    for name, (argtypes, restype) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.argtypes = argtypes
        fn.restype = restype
    if lib.gnsship_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{path}: ABI version {lib.gnsship_abi_version()}, these bindings need {ABI_VERSION} (rebuild with `make`)")
    _LIB = lib
    return lib


def check(rc: int, what: str, ctx=None) -> None:
    if rc != OK:
        msg = what
        if ctx is not None:
            detail = load().gnsship_last_error(ctx)
            if detail:
                msg = f"{what} ({detail.decode(errors='replace')})"
        raise GnssHipError(rc, msg)


def fptr(a: np.ndarray):
    return a.ctypes.data_as(_f32p)


def rotator_dispatch() -> int:
    """The volk_gnsssdr rotator variant the reference would run on this host (gnsship_rotator_dispatch):
    ROTATOR_GENERIC or ROTATOR_AVX.  Host-only: no device needed.  Raises for a preferences entry
    naming a variant the engine does not reproduce (the message says which)."""
    v = ctypes.c_int(-1)
    rc = load().gnsship_rotator_dispatch(ctypes.byref(v))
    if rc != OK:
        raise GnssHipError(rc, f"gnsship_rotator_dispatch ({rotator_dispatch_detail()})")
    return v.value


def rotator_dispatch_detail() -> str:
    buf = ctypes.create_string_buffer(512)
    load().gnsship_rotator_dispatch_detail(buf, 512)
    return buf.value.decode(errors="replace")
