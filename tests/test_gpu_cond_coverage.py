"""The signal conditioner (cond_xlating_fir.hip) on the device where tests/test_gpu_cond.py does not reach, against the
float64 model of tests/cond_model.py; the cases are those of tests/cond_coverage_cases.py, whose conditions
tests/test_cond_coverage_cases.py asserts on the model alone.

Contract, the project's: every output within (T + 8)·2⁻²³·Σ_i |h[i]|·|x[kD − i]| of the model (contract_ratio ≤ 1);
call cuts and the band mix change no bit.

* asymmetric taps: the kernel indexes z[−i]; with symmetric taps a mirrored window passes, with these the model fed the
  reversed taps misses the bound by orders of magnitude;
* the extremes of the rate: fs = 2³¹ − 1, where rr + step_mod and fc_mod·(n mod fs) come closest to 2³² and 2⁶⁴, with
  first samples up to the 2⁶² − 1 that gnsship_cond_reset admits; fs = 1, where every phase is 0;
* decimations one below, at and one above the tile length (taken from the formula of gnsship_cond_create, restated in
  cond_coverage_cases.tile_of): tiles without an output and with exactly one;
* four bands of 1, 64, 1025 and 4096 taps in one handle against their single-band handles, whose tiles differ."""
import numpy as np
import pytest

import cond_coverage_cases as C
import cond_ingest_model as I
import cond_model as M
from gnss_sim_receiver_amd import engine

pytestmark = pytest.mark.gpu


def bits(y):
    return np.ascontiguousarray(y, np.complex64).view(np.uint32)


def cut(raw, a, b):
    per = 1 if raw.dtype == np.complex64 else 2
    return raw[a * per: b * per]


def run_one(ctx, fs, band, raw, n, first=0, fmt=None):
    c = engine.SignalConditioner(ctx, fs, [band], n)
    c.reset(first)
    (y,) = c.run(raw, fmt=fmt)
    assert c.samples_in() == first + n
    c.close()
    return y


@pytest.mark.parametrize("T", C.ASYM_T)
@pytest.mark.parametrize("fmt", C.ASYM_FORMATS)
def test_asymmetric_taps(ctx, fmt, T):
    raw, x = C.stream(fmt)
    h = C.asymmetric_taps(T)
    for D in C.ASYM_D:
        y = run_one(ctx, M.FS, (C.FC, D, h), raw, M.N_IN)
        r = M.contract_ratio(y, *M.model(x, h, D, C.FC, M.FS), T)
        print(f"{fmt} T {T} D {D}: |err| / contract bound {r:.3f}")
        assert len(y) == M.N_IN // D and r <= 1.0, (fmt, T, D, r)


@pytest.mark.parametrize("T", C.RATE_T)
@pytest.mark.parametrize("fmt", ["cf32", "ci16"])
def test_largest_rate(ctx, fmt, T):
    """fs = 2³¹ − 1: fc of 1, fs − 1, −(fs − 1) and fs + 12345 Hz, first samples 0, 2³¹ + 12345 and 2⁶² − 1 − n."""
    fs, D, n = C.FS_MAX, C.RATE_D, M.N_IN
    raw, x = C.stream(fmt)
    h = C.asymmetric_taps(T)
    bnd = M.bound(x, h, D)
    worst = 0.0
    for fc in C.rate_fcs():
        c = engine.SignalConditioner(ctx, fs, [(fc, D, h)], n)
        for first in C.rate_firsts(n):
            c.reset(first)
            (y,) = c.run(raw)
            assert c.samples_in() == first + n
            r = M.contract_ratio(y, M.model_mix_fir(x, h, D, fc, fs, first), bnd, T)
            worst = max(worst, r)
            assert r <= 1.0, (fmt, T, fc, first, r)
        c.close()
    print(f"{fmt} T {T} fs 2^31 - 1: worst |err| / contract bound {worst:.3f}")


@pytest.mark.parametrize("T", C.RATE_T)
@pytest.mark.parametrize("fmt,fc", [("cf32", C.FS_MAX + 12345), ("ci8", -(C.FS_MAX - 1))])
def test_call_split_invariance_at_the_largest_rate(ctx, fmt, fc, T):
    fs, D, n = C.FS_MAX, C.RATE_D, M.N_IN
    raw, x = C.stream(fmt)
    h = C.asymmetric_taps(T)
    c = engine.SignalConditioner(ctx, fs, [(fc, D, h)], n)
    cuts = [0, D, 7 * D, 1000 * D, 1001 * D, n]
    for first in C.rate_firsts(n):
        c.reset(first)
        (whole,) = c.run(raw)
        c.reset(first)
        parts = [c.run(cut(raw, a, b))[0] for a, b in zip(cuts[:-1], cuts[1:])]
        assert c.samples_in() == first + n
        assert np.array_equal(bits(np.concatenate(parts)), bits(whole)), (fmt, T, first)
    c.close()


@pytest.mark.parametrize("T", C.RATE_T)
@pytest.mark.parametrize("name", ("cf32", "ci16", "ci8") + I.FORMATS)
def test_unit_rate_has_no_phase(ctx, name, T):
    """fs = 1: frac(fc·n/fs) = 0 for every n, so fc = 5 gives what fc = 0 gives — bit for bit for the real and the
    packed items; for the complex items as numbers, since the mix by (1, −0) may change the sign of a zero."""
    D, n = C.RATE_D, M.N_IN
    if name in ("cf32", "ci16", "ci8"):
        (raw, x), fmt = C.stream(name), None
    else:
        (raw, x), fmt = I.stream(name, n), I.fmt_value(name)
    h = C.asymmetric_taps(T)
    y0 = run_one(ctx, 1, (0, D, h), raw, n, first=12345, fmt=fmt)
    y5 = run_one(ctx, 1, (5, D, h), raw, n, first=12345, fmt=fmt)
    if fmt is None:
        assert np.array_equal(y5, y0)
    else:
        assert np.array_equal(bits(y5), bits(y0))
    assert np.any(y5 != 0)
    assert M.contract_ratio(y5, *M.model(x, h, D, 5, 1, 12345), T) <= 1.0


@pytest.mark.parametrize("T", [64, 1026])
def test_decimation_against_the_tile(ctx, T):
    """The tile length comes from the formula in gnsship_cond_create (cond_coverage_cases.tile_of: 2048 − 63 = 1985 for
    T = 64, 8192 − 1025 = 7167 for T = 1026).  n = 4·D: tiles with no output, with one, and an output on a tile's first
    and last sample."""
    h = C.asymmetric_taps(T)
    for i, D in enumerate(C.tile_decimations(T)):
        fmt = ("ci16", "cf32", "ci8")[i % 3]
        n = 4 * D
        raw, x = C.stream(fmt, n, seed=30 + i)
        y = run_one(ctx, M.FS, (C.FC, D, h), raw, n)
        r = M.contract_ratio(y, *M.model(x, h, D, C.FC, M.FS), T)
        print(f"T {T} tile {C.tile_of(T)} D {D} {fmt}: outputs per tile {C.outputs_per_tile(T, D, n).tolist()}, |err| / bound {r:.3f}")
        assert len(y) == 4 and r <= 1.0, (T, D, r)
        # the same in calls of D samples: one output to a call, the history longer or shorter than the call
        c = engine.SignalConditioner(ctx, M.FS, [(C.FC, D, h)], n)
        parts = [c.run(cut(raw, a, a + D))[0] for a in range(0, n, D)]
        c.close()
        assert np.array_equal(bits(np.concatenate(parts)), bits(y)), (T, D)


@pytest.mark.parametrize("fmt", ["cf32", "ci8"])
def test_four_bands_of_unlike_length(ctx, fmt):
    n = M.N_IN
    raw, x = C.stream(fmt)
    bands = C.four_bands()
    assert [len(b[2]) for b in bands] == [1, 64, 1025, 4096]
    first = 2**31 + 12345
    four = engine.SignalConditioner(ctx, M.FS, bands, n)
    singles = [engine.SignalConditioner(ctx, M.FS, [b], n) for b in bands]
    for c in [four] + singles:
        c.reset(first)
    got = [[] for _ in bands]
    for a, b in zip(C.FOUR_CUTS[:-1], C.FOUR_CUTS[1:]):
        ys = four.run(cut(raw, a, b))
        for i, s in enumerate(singles):
            (y1,) = s.run(cut(raw, a, b))
            assert len(ys[i]) == (b - a) // bands[i][1]
            assert np.array_equal(bits(ys[i]), bits(y1)), (fmt, a, b, i)
            got[i].append(ys[i])
    four.reset(first)
    whole = four.run(raw)
    for i, (fc, D, h) in enumerate(bands):
        assert np.array_equal(bits(np.concatenate(got[i])), bits(whole[i])), (fmt, i)
        r = M.contract_ratio(whole[i], *M.model(x, h, D, fc, M.FS, first), len(h))
        print(f"{fmt} band {i} (T {len(h)}, D {D}, fc {fc}): |err| / contract bound {r:.3f}")
        assert r <= 1.0, (fmt, i, r)
    for c in [four] + singles:
        c.close()
