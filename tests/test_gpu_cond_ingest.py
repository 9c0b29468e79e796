"""The signal conditioner's real-sampled and bit-packed input items on the GPU (cond_xlating_fir.hip,
GNSSHIP_FMT_RF32 / RI16 / RI8 and GNSSHIP_FMT_PACKED) against tests/cond_ingest_model.py and tests/cond_model.py:
rf32, ri16, ri8 and every preset of the reference's packed file sources (both byte orders of the 2-bit real form,
iq and qi).  Packed streams are random bytes, so every code occurs and the orders are distinguishable.

Contract: every output within (T + 8)·2⁻²³·Σ_i |h[i]|·|x[kD − i]| of the float64 model fed the unpacked stream; a
real stream bit-identical to the complex run of (x, 0), a packed stream to the RI8 / CI8 run of its unpacked
values; the identity filter exact; the same stream cut into calls at multiples of lcm(D, samples per byte)
bit-identical to one call, from a device pointer inside a buffer too; a multi-band handle bit-identical to
single-band handles; a misaligned n_in refused with the stream untouched; the engines refuse the new values."""
import numpy as np
import pytest

import cond_ingest_model as I
import cond_model as M
from gnss_sim_receiver_amd import abi, engine

pytestmark = pytest.mark.gpu

FIRST = 2**31 + 12345
N = I.N_IN


def run_whole(ctx, name, bands, first=0, n=N):
    raw, _ = I.stream(name, n)
    c = engine.SignalConditioner(ctx, M.FS, bands, n)
    c.reset(first)
    ys = c.run(raw, fmt=I.fmt_value(name))
    assert c.samples_in() == first + n
    c.close()
    return ys


@pytest.mark.parametrize("first", M.FIRSTS)
@pytest.mark.parametrize("name", I.FORMATS)
def test_model_parity(ctx, name, first):
    raw, x = I.stream(name)
    worst = 0.0
    for T in (1, 64, 1026):
        for D in (1, 5):
            h = M.windowed_sinc_taps(T, D)
            bnd = M.bound(x, h, D)
            for fc in (0, -7_161_000):
                (y,) = run_whole(ctx, name, [(fc, D, h)], first)
                assert len(y) == N // D
                r = M.contract_ratio(y, M.model_mix_fir(x, h, D, fc, M.FS, first), bnd, T)
                worst = max(worst, r)
                assert r <= 1.0, (name, T, D, fc, r)
    print(f"{name} first {first}: worst |err| / contract bound {worst:.3f}")


@pytest.mark.parametrize("name", I.FORMATS)
def test_exact_against_the_existing_paths(ctx, name):
    """Real: the same handle run on the CF32 / CI16 / CI8 stream (x, 0).  Packed: the RI8 (real) or CI8 (complex)
    run of the numpy-unpacked values.  Equal as numbers (signs of zero may differ), for both kernel forms."""
    raw, x = I.stream(name)
    fmt = I.fmt_value(name)
    if name == "rf32":
        other, ofmt = x, abi.FMT_CF32
    elif name in ("ri16", "ri8"):
        other = np.zeros(2 * N, raw.dtype)
        other[0::2] = raw
        ofmt = abi.FMT_CI16 if name == "ri16" else abi.FMT_CI8
    else:
        other, ofmt = I.unpack_int8(raw, fmt), (abi.FMT_RI8 if I.is_real(fmt) else abi.FMT_CI8)
        assert other.dtype == np.int8 and len(other) == (N if I.is_real(fmt) else 2 * N)
    for T, D, fc in ((64, 5, -7_161_000), (1026, 1, -7_161_000), (255, 5, 0)):
        h = M.windowed_sinc_taps(T, D)
        c = engine.SignalConditioner(ctx, M.FS, [(fc, D, h)], N)
        for first in (0, FIRST):
            c.reset(first)
            (a,) = c.run(raw, fmt=fmt)
            c.reset(first)
            (b,) = c.run(other, fmt=ofmt)
            assert np.array_equal(a, b), (name, T, D, fc, first)
        c.close()


@pytest.mark.parametrize("name", I.FORMATS)
def test_identity_filter_returns_the_unpacked_values_exactly(ctx, name):
    raw, x = I.stream(name)
    c = engine.SignalConditioner(ctx, M.FS, [(0, 1, np.ones(1, np.float32))], N)
    (y,) = c.run(raw, fmt=I.fmt_value(name))     # n_in from the array: bytes × samples per byte
    c.close()
    assert len(y) == N and np.array_equal(y, x)


@pytest.mark.parametrize("T", [255, 1026])
@pytest.mark.parametrize("name", I.FORMATS)
def test_cut_invariance(ctx, name, T):
    """One run equals the same stream cut at multiples of lcm(D, 4); T = 1026 takes the 32-register form.  The
    last round reads the cuts from a device buffer that holds the stream 64 bytes in."""
    raw, x = I.stream(name)
    fmt = I.fmt_value(name)
    D, fc = 5, -7_161_000
    h = M.windowed_sinc_taps(T, D)
    cuts = [0, 20, 140, 2000, 2020, N]
    c = engine.SignalConditioner(ctx, M.FS, [(fc, D, h)], N)
    buf = engine.DeviceBuffer(ctx, 64 + raw.nbytes)
    buf.upload(np.concatenate([np.full(64, 0xA5, np.uint8), raw.view(np.uint8)]))
    bits = ctx.lib.gnsship_cond_fmt_bits(fmt)
    for first in M.FIRSTS:
        c.reset(first)
        (whole,) = c.run(raw, fmt=fmt)
        assert M.contract_ratio(whole, *M.model(x, h, D, fc, M.FS, first), T) <= 1.0
        c.reset(first)
        parts = [c.run(I.cut(name, raw, a, b), fmt=fmt)[0] for a, b in zip(cuts[:-1], cuts[1:])]
        assert c.samples_in() == first + N
        assert np.array_equal(np.concatenate(parts), whole), (name, first)
        c.reset(first)
        parts = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            assert (a * bits) % 8 == 0
            ((ptr, n_out),) = c.run(buf.ptr + 64 + a * bits // 8, fmt=fmt, on_device=True, n_in=b - a)
            ctx.sync()
            parts.append(engine.DeviceBuffer.wrap(ctx, ptr, 8 * n_out).download(np.empty(n_out, np.complex64)))
        assert np.array_equal(np.concatenate(parts), whole), (name, first, "device pointer")
    c.close()
    buf.free()


@pytest.mark.parametrize("name", ["two_bit_packed_real_lsb", "nsr", "ri8"])
def test_multi_band_equals_single_band_handles(ctx, name):
    fs, n = 16_000_000, 8000
    raw, x = I.stream(name, n, seed=5)
    fmt = I.fmt_value(name)
    bands = [(4_000_000, 4, engine.cond_lowpass_taps(ctx.lib, fs, 4)), (-4_000_000, 2, engine.cond_lowpass_taps(ctx.lib, fs, 2))]
    both = engine.SignalConditioner(ctx, fs, bands, n)
    singles = [engine.SignalConditioner(ctx, fs, [b], n) for b in bands]
    cuts = [0, 3000, 3004, n]
    for first in (0, 123457):
        for c in [both] + singles:
            c.reset(first)
        for a, b in zip(cuts[:-1], cuts[1:]):
            ys = both.run(I.cut(name, raw, a, b), fmt=fmt)
            for i, s in enumerate(singles):
                (y1,) = s.run(I.cut(name, raw, a, b), fmt=fmt)
                assert len(ys[i]) == (b - a) // bands[i][1]
                assert np.array_equal(ys[i], y1), (first, a, b, i)
    for i, (fc, D, h) in enumerate(bands):
        both.reset(0)
        assert M.contract_ratio(both.run(raw, fmt=fmt)[i], *M.model(x, h, D, fc, fs), len(h)) <= 1.0
    for c in [both] + singles:
        c.close()


@pytest.mark.parametrize("name", ["two_bit_packed_real_msb", "two_bit_cpx", "nsr"])
def test_misaligned_n_in_is_refused_and_the_stream_continues(ctx, name):
    """n_in a multiple of D but not of the samples per byte: E_INVAL, and the next valid run continues the stream
    as if the call had not happened."""
    raw, x = I.stream(name)
    fmt = I.fmt_value(name)
    spb = I.samples_per_byte(fmt)
    D = 5
    h = M.windowed_sinc_taps(64, D)
    c = engine.SignalConditioner(ctx, M.FS, [(1_250_000, D, h)], N)
    ref = engine.SignalConditioner(ctx, M.FS, [(1_250_000, D, h)], N)
    (a,) = c.run(I.cut(name, raw, 0, 1000), fmt=fmt)
    (b,) = ref.run(I.cut(name, raw, 0, 1000), fmt=fmt)
    bad = [k * D for k in (1, 2, 3) if (k * D) % spb != 0]       # 5, 10, 15 (four per byte) or 5, 15 (two per byte)
    assert len(bad) >= 2
    for n_in in bad:
        with pytest.raises(abi.GnssHipError) as e:
            c.run(I.cut(name, raw, 1000, 1000 + 4 * D * spb), fmt=fmt, n_in=n_in)
        assert e.value.code == abi.E_INVAL and "samples per byte" in str(e.value), str(e.value)
        assert c.samples_in() == 1000
    (a2,) = c.run(I.cut(name, raw, 1000, N), fmt=fmt)
    (b2,) = ref.run(I.cut(name, raw, 1000, N), fmt=fmt)
    assert np.array_equal(a, b) and np.array_equal(a2, b2)
    c.close()
    ref.close()


def test_unknown_format_values_are_refused(ctx):
    c = engine.SignalConditioner(ctx, M.FS, [(0, 1, np.ones(1, np.float32))], 64)
    raw = np.zeros(64, np.uint8)
    for bad in (6, 7, 0x100, 0x100 | (3 << 4), 0x100 | (2 << 4) | (3 << 2), 0x200 | (2 << 4)):
        with pytest.raises(abi.GnssHipError) as e:
            c.run(raw, fmt=bad, n_in=64)
        assert e.value.code == abi.E_INVAL and "unknown sample format" in str(e.value)
        assert c.samples_in() == 0
    c.close()


def test_the_engines_refuse_the_new_formats(ctx):
    """fmt_bytes() is 0 for every new value: acquisition, tracking and the acquisition resampler keep reading
    CF32 / CI16 / CI8 only."""
    new = sorted({I.fmt_value(name) for name in I.FORMATS})
    assert len(new) == 12
    buf = engine.DeviceBuffer(ctx, 8 * 4000)
    buf.upload(np.zeros(4000, np.complex64))
    acq = engine.PcpsAcquisition(ctx, 4_000_000, 4000, 5000, 250, 0, True)
    acq.set_local_code(np.ones(4000, np.complex64))
    trk = engine.DllPllVemlTracking(ctx, abi.TrkConf.defaults(abi.SYS_GPS_L1CA, 4e6, 4000), 1)
    rs = engine.AcqResampler(ctx, np.ones(4, np.float32), 2, 4000)
    for fmt in new:
        with pytest.raises(abi.GnssHipError) as e:
            acq.run(buf, fmt=fmt)
        assert e.value.code == abi.E_INVAL, hex(fmt)
        with pytest.raises(abi.GnssHipError) as e:
            trk.run(buf, 0, 1, fmt=fmt, n_buffer_samples=4000)
        assert e.value.code == abi.E_INVAL, hex(fmt)
        with pytest.raises(abi.GnssHipError) as e:
            rs.run(buf.ptr, fmt=fmt, on_device=True, n_in=4000)
        assert e.value.code == abi.E_INVAL, hex(fmt)
    acq.run(buf, fmt=abi.FMT_CF32)     # the handles are still good
    acq.close()
    trk.close()
    rs.close()
    buf.free()
