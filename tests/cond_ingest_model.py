"""Numpy model of the signal conditioner's real-sampled and bit-packed input items (GNSSHIP_FMT_RF32 /
RI16 / RI8 and GNSSHIP_FMT_PACKED, include/gnsship.h), beside tests/cond_model.py: the converted stream goes
through cond_model.model_mix_fir unchanged, a real x being complex with a zero imaginary part.

Two unpackers, written independently:

* :func:`unpack` from the generic description — a byte holds F = 8/bits fields; field j in stream order sits
  at bit offset bits·j (LSB first) or 8 − bits·(j + 1) (MSB first) and is a two's-complement integer s; the
  value is 2s + 1 or s; REAL takes one field per sample, IQ fields 2m, 2m + 1 as (re, im), QI as (im, re).
* ``ref_*`` — literal restatements of the reference's unpacking loops (same shifts, masks and output order).

How each preset follows from the reference (derived from the cited lines, checked by test_cond_ingest_model):

Two_Bit_Packed, byte items (unpack_2bit_samples.cc).  The byte is read through a union with four ``signed :2``
bit-fields sample_0..sample_3 (:22-35); GCC and Clang on a little-endian host allocate bit-fields from the
least significant bit, so sample_k is bits 2k+1:2k as a two's-complement integer.  systemBytesAreBigEndian()
(:50-60) stores 1 in the byte and reads the same byte back, so it is false on every host, and
swap_endian_bytes_ = big_endian_bytes (:117-119).  Without the swap the output order is sample_0, 1, 2, 3
(:167-176): LSB first; with it sample_3, 2, 1, 0 (:154-163): MSB first.  Every value is 2·sample + 1.
sample_type "real" makes one float per value; "iq" feeds interleaved_char_to_complex, (even, odd) = (re, im)
(two_bit_packed_file_signal_source.cc:79-91,119-131); "qi" sets reverse_interleaving, which swaps each pair of
the output order (:179-206: sample_1, 0, 3, 2, or with the byte swap sample_2, 3, 0, 1), so in either field
order fields 2m, 2m + 1 are (im, re).  The adapter's defaults are "real" and big_endian_bytes false (:33-36).

Nsr (unpack_byte_2bit_samples.cc:50-65): c & 3, (c >> 2) & 3, (c >> 4) & 3, (c >> 6) & 3 in that order, each
stored in a ``signed :2`` bit-field and converted to float as it is: 2 bits, REAL, LSB first, value s.

Two_Bit_Cpx (unpack_byte_2bit_cpx_samples.cc:77-90): the shorts come out as (c >> 4) & 3, (c >> 6) & 3, c & 3,
(c >> 2) & 3, each 2s + 1.  two_bit_cpx_file_signal_source.cc:69 follows with
interleaved_short_to_complex(false, true).  GNU Radio is not in the reference tree; the block's second
argument, swap, is restated from its published meaning: with swap the second short of a pair is the real
part.  So re = bits 7:6, im = bits 5:4, then re = 3:2, im = 1:0: 2 bits, IQ, MSB first, 2s + 1.

Four_Bit_Cpx (unpack_byte_4bit_samples.cc:44-65): the low nibble first, then the high one, each t ≥ 8 →
2(t − 16) + 1, else 2t + 1, i.e. 2s + 1 of the 4-bit two's-complement s; then
interleaved_short_to_complex(false, reverse_interleaving) with reverse_interleaving = (sample_type == "qi"),
default "iq" (four_bit_cpx_file_signal_source.cc:33-50,108): 4 bits, IQ / QI, LSB first, 2s + 1.
"""
import numpy as np

from gnss_sim_receiver_amd import abi

import cond_model as M

N_IN = M.N_IN

# name -> (format value, literal reference unpacker)
PRESETS = {}


def fields_per_byte(fmt):
    return 8 // abi.fmt_packed_fields(fmt)[0]


def samples_per_byte(fmt):
    bits, comp, _, _ = abi.fmt_packed_fields(fmt)
    return 8 // bits if comp == abi.PACKED_REAL else 4 // bits


def is_real(fmt):
    return fmt in (abi.FMT_RF32, abi.FMT_RI16, abi.FMT_RI8) or (abi.fmt_is_packed(fmt) and abi.fmt_packed_fields(fmt)[1] == abi.PACKED_REAL)


# ---- the generic description ----

def unpack_fields(raw, fmt) -> np.ndarray:
    """The field values of a packed byte stream in stream order (int8), value map applied."""
    bits, _, order, vmap = abi.fmt_packed_fields(fmt)
    f = 8 // bits
    b = np.asarray(raw, np.uint8).astype(np.int32)
    j = np.arange(f)
    off = bits * j if order == abi.PACKED_LSB_FIRST else 8 - bits * (j + 1)
    u = (b[:, None] >> off[None, :]) & ((1 << bits) - 1)
    s = u - ((u >> (bits - 1)) << bits)
    v = 2 * s + 1 if vmap == abi.PACKED_MAP_2S1 else s
    return v.reshape(-1).astype(np.int8)


def unpack_int8(raw, fmt) -> np.ndarray:
    """The stream as the RI8 (real) or CI8 (complex: interleaved re, im) items holding the same values."""
    v = unpack_fields(raw, fmt)
    if abi.fmt_packed_fields(fmt)[1] == abi.PACKED_QI:
        v = v.reshape(-1, 2)[:, ::-1].reshape(-1)
    return np.ascontiguousarray(v)


def unpack(raw, fmt) -> np.ndarray:
    """The stream as complex64 samples (imaginary part 0 for REAL)."""
    v = unpack_int8(raw, fmt).astype(np.float32)
    if abi.fmt_packed_fields(fmt)[1] == abi.PACKED_REAL:
        return v.astype(np.complex64)
    return np.ascontiguousarray(v).view(np.complex64)


def pack(values, fmt) -> np.ndarray:
    """Inverse of unpack_fields: field values (after the value map) in stream order -> bytes."""
    bits, _, order, vmap = abi.fmt_packed_fields(fmt)
    f = 8 // bits
    v = np.asarray(values, np.int64)
    if vmap == abi.PACKED_MAP_2S1:
        assert np.all(v % 2 != 0)
        s = (v - 1) // 2
    else:
        s = v
    assert np.all((s >= -(1 << (bits - 1))) & (s < (1 << (bits - 1)))) and len(s) % f == 0
    u = (s & ((1 << bits) - 1)).reshape(-1, f)
    j = np.arange(f)
    off = bits * j if order == abi.PACKED_LSB_FIRST else 8 - bits * (j + 1)
    return np.bitwise_or.reduce(u << off[None, :], axis=1).astype(np.uint8)


def pack_samples(x, fmt) -> np.ndarray:
    """Samples (real array, or complex with integer parts) -> packed bytes of the format."""
    comp = abi.fmt_packed_fields(fmt)[1]
    if comp == abi.PACKED_REAL:
        return pack(np.rint(np.real(x)).astype(np.int64), fmt)
    x = np.asarray(x, np.complex128)
    pair = (x.real, x.imag) if comp == abi.PACKED_IQ else (x.imag, x.real)
    return pack(np.rint(np.stack(pair, axis=1).reshape(-1)).astype(np.int64), fmt)


def quantise_2bit(r, sigma) -> np.ndarray:
    """A real stream quantised to 2 bits with thresholds at 0 and ±σ: values ±1 and ±3."""
    r = np.asarray(r, np.float64)
    return (np.where(np.abs(r) > sigma, 3, 1) * np.where(r >= 0, 1, -1)).astype(np.int8)


# ---- literal restatements of the reference's loops ----

def _signed2(u):
    """Assignment to a `signed :2` bit-field: the low two bits as a two's-complement integer."""
    u = np.asarray(u, np.int32) & 3
    return np.where(u >= 2, u - 4, u)


def _interleaved_to_complex(v, swap=False):
    """interleaved_char_to_complex(false) / interleaved_short_to_complex(false, swap), restated from the
    blocks' published meaning: pairs (first, second) -> first + j·second, or with swap second + j·first."""
    v = np.asarray(v, np.float32).reshape(-1, 2)
    re, im = (v[:, 1], v[:, 0]) if swap else (v[:, 0], v[:, 1])
    return (re + 1j * im).astype(np.complex64)


def ref_two_bit_packed(raw, sample_type="real", big_endian_bytes=False):
    """unpack_2bit_samples.cc:150-207 with item_size 1 on a little-endian host, then the source's
    char-to-float / interleaved_char_to_complex (two_bit_packed_file_signal_source.cc:119-131)."""
    c = np.asarray(raw, np.uint8).astype(np.int32)
    sample = [_signed2(c >> (2 * k)) for k in range(4)]            # byte_2bit_struct sample_0 .. sample_3
    swap_endian_bytes = bool(big_endian_bytes)                     # systemBytesAreBigEndian() is false
    reverse_interleaving = sample_type == "qi"
    if not reverse_interleaving:
        order = (3, 2, 1, 0) if swap_endian_bytes else (0, 1, 2, 3)    # :159-162 / :172-175
    else:
        order = (2, 3, 0, 1) if swap_endian_bytes else (1, 0, 3, 2)    # :188-191 / :201-204
    out = np.stack([2 * sample[k] + 1 for k in order], axis=1).reshape(-1)
    if sample_type == "real":
        return out.astype(np.float32).astype(np.complex64)
    return _interleaved_to_complex(out)


def ref_nsr(raw):
    """unpack_byte_2bit_samples.cc:50-65."""
    c = np.asarray(raw, np.uint8).view(np.int8).astype(np.int32)   # signed char c = in[i]
    out = np.stack([_signed2(c & 3), _signed2((c >> 2) & 3), _signed2((c >> 4) & 3), _signed2((c >> 6) & 3)], axis=1).reshape(-1)
    return out.astype(np.float32).astype(np.complex64)


def ref_two_bit_cpx(raw):
    """unpack_byte_2bit_cpx_samples.cc:77-90, then interleaved_short_to_complex(false, true)
    (two_bit_cpx_file_signal_source.cc:69; swap = the second short is the real part)."""
    c = np.asarray(raw, np.uint8).view(np.int8).astype(np.int32)   # int8_t c = in[i]
    out = np.stack([2 * _signed2((c >> 4) & 3) + 1, 2 * _signed2((c >> 6) & 3) + 1, 2 * _signed2(c & 3) + 1, 2 * _signed2((c >> 2) & 3) + 1],
                   axis=1).reshape(-1)
    return _interleaved_to_complex(out, swap=True)


def ref_four_bit_cpx(raw, sample_type="iq"):
    """unpack_byte_4bit_samples.cc:44-65, then interleaved_short_to_complex(false, reverse_interleaving)
    (four_bit_cpx_file_signal_source.cc:38-50,108)."""
    b = np.asarray(raw, np.uint8).astype(np.int32)

    def nibble(t):
        return np.where(t >= 8, 2 * (t - 16) + 1, 2 * t + 1)

    out = np.stack([nibble(b & 0x0F), nibble((b >> 4) & 0x0F)], axis=1).reshape(-1)
    return _interleaved_to_complex(out, swap=(sample_type == "qi"))


for _t in ("real", "iq", "qi"):
    for _be in (False, True):
        PRESETS[f"two_bit_packed_{_t}_{'msb' if _be else 'lsb'}"] = (
            abi.fmt_two_bit_packed(_t, _be), lambda raw, t=_t, be=_be: ref_two_bit_packed(raw, t, be))
PRESETS["nsr"] = (abi.FMT_NSR, ref_nsr)
PRESETS["two_bit_cpx"] = (abi.FMT_TWO_BIT_CPX, ref_two_bit_cpx)
PRESETS["four_bit_cpx_iq"] = (abi.fmt_four_bit_cpx("iq"), lambda raw: ref_four_bit_cpx(raw, "iq"))
PRESETS["four_bit_cpx_qi"] = (abi.fmt_four_bit_cpx("qi"), lambda raw: ref_four_bit_cpx(raw, "qi"))

REAL_FORMATS = {"rf32": abi.FMT_RF32, "ri16": abi.FMT_RI16, "ri8": abi.FMT_RI8}
# every new input form of the GPU tests
FORMATS = tuple(REAL_FORMATS) + tuple(PRESETS)

_STREAMS = {}


def fmt_value(name):
    return REAL_FORMATS[name] if name in REAL_FORMATS else PRESETS[name][0]


def stream(name, n=N_IN, seed=21):
    """(raw, x): n samples of the named input form and the same samples as complex64 exactly as the load
    converts them.  Real forms: seeded noise; packed forms: random bytes, so every code occurs."""
    key = (name, n, seed)
    if key not in _STREAMS:
        rng = np.random.default_rng(seed)
        if name == "rf32":
            raw = (rng.standard_normal(n) * 6).astype(np.float32)
            x = raw.astype(np.complex64)
        elif name in ("ri16", "ri8"):
            scale, dt = (3000.0, np.int16) if name == "ri16" else (20.0, np.int8)
            info = np.iinfo(dt)
            raw = np.clip(np.rint(rng.standard_normal(n) * scale), info.min, info.max).astype(dt)
            x = raw.astype(np.float32).astype(np.complex64)
        else:
            fmt = PRESETS[name][0]
            assert n % samples_per_byte(fmt) == 0
            raw = rng.integers(0, 256, n // samples_per_byte(fmt), dtype=np.uint8)
            x = unpack(raw, fmt)
        _STREAMS[key] = (raw, x)
    return _STREAMS[key]


def cut(name, raw, a, b):
    """Samples [a, b) of a raw stream of the named form (a, b multiples of the samples per byte)."""
    if name in REAL_FORMATS:
        return raw[a:b]
    spb = samples_per_byte(PRESETS[name][0])
    assert a % spb == 0 and b % spb == 0
    return raw[a // spb: b // spb]
