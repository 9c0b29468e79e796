"""The conditioner's real-sampled and bit-packed input items, host side (no GPU): the generic unpacker of
tests/cond_ingest_model.py against the literal restatements of the reference's unpacking loops, the packers
the other tests use, the format values, and the bits-per-sample helper of the C ABI."""
import numpy as np
import pytest

import cond_ingest_model as I
import cond_model as M
from gnss_sim_receiver_amd import abi, engine


@pytest.mark.parametrize("name", list(I.PRESETS))
def test_generic_unpacker_equals_the_reference_loop(name):
    fmt, ref = I.PRESETS[name]
    every = np.arange(256, dtype=np.uint8)
    rnd = np.random.default_rng(3).integers(0, 256, 4096, dtype=np.uint8)
    for raw in (every, rnd):
        got, want = I.unpack(raw, fmt), ref(raw)
        assert got.dtype == want.dtype == np.complex64 and len(got) == len(raw) * I.samples_per_byte(fmt)
        assert np.array_equal(got, want), name
    # the named bit positions of the issue's table, on one byte: 0b10_01_11_00
    b = np.array([0b10011100], np.uint8)
    if name == "two_bit_cpx":          # re = bits 7:6, im = 5:4, then 3:2, 1:0; value 2s + 1
        assert list(I.unpack(b, fmt)) == [-3 + 3j, -1 + 1j]
    if name == "nsr":                  # LSB first, value s
        assert list(I.unpack(b, fmt).real) == [0, -1, 1, -2]
    if name == "two_bit_packed_real_lsb":
        assert list(I.unpack(b, fmt).real) == [1, -1, 3, -3]
    if name == "two_bit_packed_real_msb":
        assert list(I.unpack(b, fmt).real) == [-3, 3, -1, 1]
    if name == "two_bit_packed_qi_lsb":
        assert list(I.unpack(b, fmt)) == [-1 + 1j, -3 + 3j]
    if name == "four_bit_cpx_iq":      # low nibble 0b1100 = −4 → −7, high 0b1001 = −7 → −13
        assert list(I.unpack(b, fmt)) == [-7 - 13j]
    if name == "four_bit_cpx_qi":
        assert list(I.unpack(b, fmt)) == [-13 - 7j]


def test_presets_are_distinct_and_distinguishable_on_random_bytes():
    """No two different presets with the same sample count per byte give the same stream: the GPU tests on
    random bytes tell a wrong field order, pair order or value map apart.  Two_Bit_Cpx and Two_Bit_Packed iq
    with big_endian_bytes are one format (2 bits, IQ, MSB first, 2s + 1) under two names."""
    vals = [f for f, _ in I.PRESETS.values()]
    assert I.PRESETS["two_bit_cpx"][0] == I.PRESETS["two_bit_packed_iq_msb"][0]
    assert len(vals) == 10 and len(set(vals)) == 9
    assert set(vals) == set(abi.PACKED_PRESETS.values())
    assert not set(vals) & {abi.FMT_CF32, abi.FMT_CI16, abi.FMT_CI8, abi.FMT_RF32, abi.FMT_RI16, abi.FMT_RI8}
    raw = I.stream("nsr")[0]
    names = list(I.PRESETS)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            if I.PRESETS[a][0] == I.PRESETS[b][0]:
                continue
            xa, xb = I.unpack(raw, I.PRESETS[a][0]), I.unpack(raw, I.PRESETS[b][0])
            assert len(xa) != len(xb) or not np.array_equal(xa, xb), (a, b)


@pytest.mark.parametrize("name", list(I.PRESETS))
def test_packers_round_trip(name):
    fmt = I.PRESETS[name][0]
    raw = I.stream(name)[0]
    assert np.array_equal(I.pack(I.unpack_fields(raw, fmt), fmt), raw)
    assert np.array_equal(I.pack_samples(I.unpack(raw, fmt), fmt), raw)
    x = I.unpack(raw, fmt)
    i8 = I.unpack_int8(raw, fmt)
    if I.is_real(fmt):
        assert np.array_equal(i8.astype(np.float32), x.real) and not x.imag.any()
    else:
        assert np.array_equal(i8.astype(np.float32).view(np.complex64), x)


def test_two_bit_quantiser_packs_to_the_four_codes():
    r = np.array([-2.5, -1.0, -0.2, 0.0, 0.3, 1.0, 1.01, 7.0])
    q = I.quantise_2bit(r, 1.0)
    assert list(q) == [-3, -1, -1, 1, 1, 1, 3, 3]
    fmt = abi.fmt_two_bit_packed("real", False)
    assert np.array_equal(I.unpack(I.pack(q, fmt), fmt).real, q)


@pytest.mark.parametrize("name", ["ri8", "two_bit_packed_real_lsb", "four_bit_cpx_qi"])
def test_converted_streams_go_through_the_model_unchanged(name):
    """A real x is complex with a zero imaginary part: the float64 model and its bound take it as it is, and the
    plain float32 formulation stays inside the contract."""
    raw, x = I.stream(name)
    assert x.dtype == np.complex64 and len(x) == I.N_IN
    T, D, fc = 64, 5, -7_161_000
    h = M.windowed_sinc_taps(T, D)
    ref, bnd = M.model(x[:2000], h, D, fc, M.FS, 2**31 + 12345)
    assert M.contract_ratio(M.f32_mix_fir(x[:2000], h, D, fc, M.FS, 2**31 + 12345), ref, bnd, T) <= 1.0
    if I.is_real(I.fmt_value(name)):
        # two multiplies instead of the complex product: the same values up to signs of zero
        p = M.phasor(fc, M.FS, np.arange(2000, dtype=np.int64)).astype(np.complex64)
        xr = x[:2000].real
        two = (xr * p.real) + 1j * -(xr * -p.imag)
        assert np.array_equal(two.astype(np.complex64), (x[:2000] * p).astype(np.complex64))


def test_bits_per_sample_helper_and_python_defaults(built):
    lib = abi.load()
    want = {abi.FMT_CF32: 64, abi.FMT_CI16: 32, abi.FMT_CI8: 16, abi.FMT_RF32: 32, abi.FMT_RI16: 16, abi.FMT_RI8: 8}
    for name, (fmt, _) in I.PRESETS.items():
        want[fmt] = 8 // I.samples_per_byte(fmt)
    want[abi.fmt_packed(4, abi.PACKED_REAL, abi.PACKED_MSB_FIRST, abi.PACKED_MAP_S)] = 4
    for fmt, bits in want.items():
        assert lib.gnsship_cond_fmt_bits(fmt) == bits, hex(fmt)
    for bad in (-1, 6, 7, 0xFF, 0x100, 0x100 | (3 << 4), 0x100 | (8 << 4), 0x100 | (2 << 4) | (3 << 2), 0x200 | (2 << 4), 1 << 20):
        assert lib.gnsship_cond_fmt_bits(bad) == 0, hex(bad)
    # sample_format() keeps inferring only the three complex formats
    assert engine.sample_format(np.zeros(2, np.complex64)) == abi.FMT_CF32
    assert engine.sample_format(np.zeros(2, np.int16)) == abi.FMT_CI16
    assert engine.sample_format(np.zeros(2, np.int8)) == abi.FMT_CI8
    for dt in (np.uint8, np.float32):
        with pytest.raises(TypeError):
            engine.sample_format(np.zeros(2, dt))
    with pytest.raises(ValueError):
        abi.fmt_packed(3, 0, 0, 0)
