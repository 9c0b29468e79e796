"""Signal conditioner on the GPU (cond_xlating_fir.hip): the streaming multi-band frequency-translating
FIR decimator against the float64 model of tests/cond_model.py
(gr::filter::freq_xlating_fir_filter_ccf restated; freq_xlating_fir_filter.cc:36-117).

Contract: every output within (T + 8)·2⁻²³·Σ_i |h[i]|·|x[kD − i]| of the model; the identity filter
exact; the same stream cut into calls anywhere at multiples of D bit-identical to one call; a multi-band
handle bit-identical to single-band handles; every rejected call leaves the stream untouched.
"""
import ctypes

import numpy as np
import pytest

import cond_model as M
from gnss_sim_receiver_amd import abi, engine

pytestmark = pytest.mark.gpu

_STREAMS = {}


def stream(fmt):
    if fmt not in _STREAMS:
        _STREAMS[fmt] = M.stream(fmt)
    return _STREAMS[fmt]


def cut(raw, a, b):
    per = 1 if raw.dtype == np.complex64 else 2
    return raw[a * per: b * per]


@pytest.mark.parametrize("first", M.FIRSTS)
@pytest.mark.parametrize("fmt", ["cf32", "ci16", "ci8"])
def test_model_parity(ctx, fmt, first):
    raw, x = stream(fmt)
    worst = 0.0
    for T in M.SHAPES_T:
        for D in M.SHAPES_D:
            h = M.windowed_sinc_taps(T, D)
            bnd = M.bound(x, h, D)
            for fc in M.SHAPES_FC:
                c = engine.SignalConditioner(ctx, M.FS, [(fc, D, h)], M.N_IN)
                c.reset(first)
                (y,) = c.run(raw)
                assert c.samples_in() == first + M.N_IN
                c.close()
                assert len(y) == M.N_IN // D
                r = M.contract_ratio(y, M.model_mix_fir(x, h, D, fc, M.FS, first), bnd, T)
                worst = max(worst, r)
                assert r <= 1.0, (T, D, fc, r)
    print(f"{fmt} first {first}: worst |err| / contract bound {worst:.3f}")


@pytest.mark.parametrize("fmt", ["cf32", "ci16", "ci8"])
def test_identity_filter_returns_the_converted_input_exactly(ctx, fmt):
    raw, x = stream(fmt)
    c = engine.SignalConditioner(ctx, M.FS, [(0, 1, np.ones(1, np.float32))], M.N_IN)
    (y,) = c.run(raw)
    c.close()
    assert np.array_equal(y, x)


@pytest.mark.parametrize("fmt,fc", [("cf32", -7_161_000), ("ci8", 1_250_000)])
def test_call_split_invariance(ctx, fmt, fc):
    raw, x = stream(fmt)
    T, D, n = 255, 5, M.N_IN
    h = M.windowed_sinc_taps(T, D)
    c = engine.SignalConditioner(ctx, M.FS, [(fc, D, h)], n)
    (whole,) = c.run(raw)
    assert M.contract_ratio(whole, *M.model(x, h, D, fc, M.FS), T) <= 1.0
    cuts = [0, D, 7 * D, 1000 * D, 1001 * D, n]
    for first in (0, 2**31 + 12345):
        c.reset(first)
        (ref,) = c.run(raw)
        if first == 0:
            assert np.array_equal(ref, whole)       # reset returns to the state after create
        c.reset(first)
        parts = [c.run(cut(raw, a, b))[0] for a, b in zip(cuts[:-1], cuts[1:])]
        assert c.samples_in() == first + n
        assert np.array_equal(np.concatenate(parts), ref), first
    c.close()


@pytest.mark.parametrize("T", [1026, 4096])
def test_filters_beyond_1025_taps_take_the_wide_span_kernel(ctx, T):
    """Above 1025 taps the span no longer fits eight samples per lane: the 32-per-lane form of the kernel
    (64 KiB of LDS) runs.  Same contract, same call-split invariance; a second, short band rides along."""
    raw, x = stream("ci16")
    D, fc, n = 2, -7_161_000, M.N_IN
    h = M.windowed_sinc_taps(T, D)
    h2 = M.windowed_sinc_taps(64, 5)
    c = engine.SignalConditioner(ctx, M.FS, [(fc, D, h), (1_250_000, 5, h2)], n)
    c.reset(2**31 + 12345)
    whole = c.run(raw)
    assert M.contract_ratio(whole[0], *M.model(x, h, D, fc, M.FS, 2**31 + 12345), T) <= 1.0
    assert M.contract_ratio(whole[1], *M.model(x, h2, 5, 1_250_000, M.FS, 2**31 + 12345), 64) <= 1.0
    c.reset(2**31 + 12345)
    cuts = [0, 10, 70, 5000, 5010, n]
    parts = [c.run(cut(raw, a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
    for i in range(2):
        assert np.array_equal(np.concatenate([p[i] for p in parts]), whole[i]), i
    c.close()


def test_multi_band_equals_single_band_handles(ctx):
    fs, n = 16_000_000, 8000
    raw, x = M.stream("ci8", n, seed=5)
    bands = [(4_000_000, 4, engine.cond_lowpass_taps(ctx.lib, fs, 4)), (-4_000_000, 2, engine.cond_lowpass_taps(ctx.lib, fs, 2))]
    assert [len(b[2]) for b in bands] == [193, 97]
    both = engine.SignalConditioner(ctx, fs, bands, n)
    singles = [engine.SignalConditioner(ctx, fs, [b], n) for b in bands]
    cuts = [0, 3000, 3004, n]   # the long-history and the short-history band cross the same call edges
    for first in (0, 123457):
        for c in [both] + singles:
            c.reset(first)
        for a, b in zip(cuts[:-1], cuts[1:]):
            ys = both.run(cut(raw, a, b))
            for i, s in enumerate(singles):
                (y1,) = s.run(cut(raw, a, b))
                assert len(ys[i]) == (b - a) // bands[i][1]
                assert np.array_equal(ys[i], y1), (first, a, b, i)
    for i, (fc, D, h) in enumerate(bands):
        both.reset(0)
        assert M.contract_ratio(both.run(raw)[i], *M.model(x, h, D, fc, fs), len(h)) <= 1.0
    # caller-supplied destinations (a slot of the caller's own device buffer) and the n_out values
    both.reset(0)
    own = both.run(raw)
    both.reset(0)
    buf = engine.DeviceBuffer(ctx, 8 * (100 + n // 4 + n // 2))
    dst = [buf.ptr + 8 * 100, None]
    src = ctx.upload(raw)
    got = both.run(src.ptr, fmt=abi.FMT_CI8, on_device=True, n_in=n, dev_dst=dst)
    assert got[0] == (dst[0], n // 4) and got[1][1] == n // 2 and got[1][0] not in (None, 0, dst[0])
    ctx.sync()
    y0 = buf.download(np.empty(n // 4, np.complex64), offset=8 * 100)
    y1 = engine.DeviceBuffer.wrap(ctx, got[1][0], 8 * (n // 2)).download(np.empty(n // 2, np.complex64))
    assert np.array_equal(y0, own[0]) and np.array_equal(y1, own[1])
    for c in [both] + singles:
        c.close()
    buf.free()
    src.free()


def test_rejections_leave_the_stream_unchanged(ctx):
    lib, h = ctx.lib, M.windowed_sinc_taps(64, 2)

    def create(fs, bands, max_in=1000):
        arr = (abi.CondBand * max(1, len(bands)))()
        keep = []
        for i, (f, d, t, nt) in enumerate(bands):
            t = np.ascontiguousarray(t, np.float32)
            keep.append(t)
            arr[i] = abi.CondBand(if_hz=f, decimation=d, taps=abi.fptr(t), n_taps=nt)
        out = ctypes.c_void_p()
        rc = lib.gnsship_cond_create(ctx.h, fs, arr, len(bands), max_in, ctypes.byref(out))
        if rc == abi.OK:
            lib.gnsship_cond_destroy(out)
        return rc, lib.gnsship_last_error(ctx.h).decode()

    ok = (1e6, 2, h, 64)
    assert create(50e6, [ok])[0] == abi.OK
    for fs, bands in [(50e6 + 0.5, [ok]),                          # non-integer fs_in
                      (50e6, [(1e6 + 0.25, 2, h, 64)]),            # non-integer if_hz
                      (50e6, [(1e6, 0, h, 64)]),                   # D < 1
                      (50e6, []),                                  # n_bands outside 1..4
                      (50e6, [ok] * 5),
                      (50e6, [(1e6, 2, h, 0)]),                    # n_taps outside 1..4096
                      (50e6, [(1e6, 2, np.zeros(4097, np.float32), 4097)])]:
        rc, msg = create(fs, bands)
        assert rc == abi.E_INVAL and msg.startswith("gnsship_cond_create"), (fs, len(bands), msg)
    assert create(50e6, [(1e6, 2, np.zeros(4096, np.float32), 4096)] * 4)[0] == abi.OK
    for max_in in (0, 1, 2**30 + 1, 2**41):                          # max_in_samples outside 1..2^30, or below a band's D
        rc, msg = create(50e6, [ok], max_in)
        assert rc == abi.E_INVAL and msg.startswith("gnsship_cond_create"), (max_in, msg)

    raw, x = stream("cf32")
    bands = [(1_250_000, 2, h), (-7_161_000, 5, M.windowed_sinc_taps(255, 5))]
    c = engine.SignalConditioner(ctx, M.FS, bands, 4000)
    ref = engine.SignalConditioner(ctx, M.FS, bands, 4000)
    a = c.run(raw[:1000])
    b = ref.run(raw[:1000])
    for bad in (raw[1000:1015], raw[1000:1004], raw[1000:1005], raw[:4010]):  # not a multiple of 10 / above max_in_samples
        with pytest.raises(abi.GnssHipError) as e:
            c.run(bad)
        assert e.value.code == abi.E_INVAL and "gnsship_cond_run" in str(e.value)
        assert c.samples_in() == 1000
    a2 = c.run(raw[1000:5000])
    b2 = ref.run(raw[1000:5000])
    for i in range(2):
        assert np.array_equal(a[i], b[i]) and np.array_equal(a2[i], b2[i])
    c.close()
    ref.close()
