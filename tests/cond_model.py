"""Float64 model of the signal conditioner's frequency-translating FIR decimator
(gr::filter::freq_xlating_fir_filter_ccf(D, taps, fc, fs), restated from its published definition; the
reference uses it through src/algorithms/input_filter/adapters/freq_xlating_fir_filter.cc:36-117).

With ω = 2π·fc/fs, T real taps h, zeros before the stream and `first` the absolute index of the
stream's first sample (the phase origin is absolute sample 0):

    y[k] = Σ_{i<T} h[i] · x[kD − i] · e^{−jω(first + kD − i)}                      (form A: mix, then FIR)
         = e^{−jω(first + kD)} · Σ_{i<T} (h[i]·e^{jωi}) · x[kD − i]                (form B: composite taps, rotator)

The phase of absolute sample n is −2π·frac(fc·n/fs), the fraction exact in integers.  Every function
returns the per-output bound Σ_i |h[i]|·|x[kD − i]| the accuracy contract scales with:

    |y − y_ref| ≤ (T + 8) · 2⁻²³ · Σ_i |h[i]|·|x[kD − i]|
"""
import numpy as np

FS = 50_000_000
SHAPES_T = (1, 5, 64, 255, 1025)
SHAPES_D = (1, 2, 5)
SHAPES_FC = (0, 1_250_000, -7_161_000)
FIRSTS = (0, 2**31 + 12345)
N_IN = 6000


def phase_frac(fc: int, fs: int, n) -> np.ndarray:
    """frac(fc·n/fs) for integer fc, fs (< 2³¹) and integer n (array), exact: ((fc mod fs)(n mod fs) mod fs)/fs."""
    fc, fs = int(fc), int(fs)
    assert 0 < fs < 2**31
    n = np.asarray(n, np.int64)
    r = (np.int64(fc % fs) * np.mod(n, np.int64(fs))) % np.int64(fs)
    return r.astype(np.float64) / float(fs)


def phasor(fc: int, fs: int, n, sign: float = -1.0) -> np.ndarray:
    """e^{sign·j2π·frac(fc·n/fs)} in complex128."""
    a = 2.0 * np.pi * phase_frac(fc, fs, n)
    return np.cos(a) + sign * 1j * np.sin(a)


def bound(x, taps, decim: int) -> np.ndarray:
    """Σ_i |h[i]|·|x[kD − i]| per output k."""
    x = np.asarray(x, np.complex128)
    h = np.asarray(taps, np.float64)
    return np.convolve(np.abs(x), np.abs(h))[: len(x)][::decim]


def model_mix_fir(x, taps, decim: int, fc: int, fs: int, first: int = 0) -> np.ndarray:
    """Form A in float64."""
    x = np.asarray(x, np.complex128)
    h = np.asarray(taps, np.float64)
    z = x * phasor(fc, fs, first + np.arange(len(x), dtype=np.int64))
    return np.convolve(z, h)[: len(x)][::decim]


def model_composite(x, taps, decim: int, fc: int, fs: int, first: int = 0) -> np.ndarray:
    """Form B in float64."""
    x = np.asarray(x, np.complex128)
    h = np.asarray(taps, np.float64)
    g = h * phasor(fc, fs, np.arange(len(h), dtype=np.int64), sign=+1.0)
    y = np.convolve(x, g)[: len(x)][::decim]
    return y * phasor(fc, fs, first + np.arange(0, len(x), decim, dtype=np.int64))


def model(x, taps, decim: int, fc: int, fs: int, first: int = 0):
    """(y_ref, bound) — the reference of the accuracy contract."""
    return model_mix_fir(x, taps, decim, fc, fs, first), bound(x, taps, decim)


def contract_ratio(y, y_ref, bnd, n_taps: int) -> float:
    """max over outputs of |y − y_ref| / ((T + 8)·2⁻²³·bound); the contract is ratio ≤ 1.  Outputs whose
    bound is 0 (all-zero window) must be exactly 0."""
    err = np.abs(np.asarray(y, np.complex128) - y_ref)
    lim = (n_taps + 8) * 2.0**-23 * bnd
    if np.any(err[lim == 0] != 0):
        return np.inf
    nz = lim > 0
    return float(np.max(err[nz] / lim[nz])) if nz.any() else 0.0


def windowed_sinc_taps(n_taps: int, decim: int) -> np.ndarray:
    """A Hamming-windowed sinc of n_taps float taps with cutoff 0.4/D of the input rate, unit DC gain
    (n_taps = 1: [1]) — a low-pass of any length, which firdes::low_pass cannot give."""
    if n_taps == 1:
        return np.ones(1, np.float32)
    m = np.arange(n_taps) - (n_taps - 1) / 2.0
    h = np.sinc(0.8 / decim * m) * (0.54 - 0.46 * np.cos(2 * np.pi * np.arange(n_taps) / (n_taps - 1)))
    return (h / h.sum()).astype(np.float32)



def stream(fmt: str, n: int = N_IN, seed: int = 20):
    """(raw, as_float): a seeded noise stream in the named IF format (cf32 / ci16 / ci8; interleaved ints)
    and the same samples as complex64 exactly as the load converts them."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    if fmt == "cf32":
        raw = (x * 6).astype(np.complex64)
        return raw, raw
    scale, dt = (20.0, np.int8) if fmt == "ci8" else (3000.0, np.int16)
    info = np.iinfo(dt)
    raw = np.empty(2 * n, dt)
    raw[0::2] = np.clip(np.rint(x.real * scale), info.min, info.max)
    raw[1::2] = np.clip(np.rint(x.imag * scale), info.min, info.max)
    return raw, raw.astype(np.float32).view(np.complex64)


# ---- plain float32 formulations (what a straightforward single-precision implementation computes) ----

def f32_mix_fir(x, taps, decim: int, fc: int, fs: int, first: int = 0) -> np.ndarray:
    """Form A with every operation rounded to float32: the phasor rounded once from double, one complex
    product per sample, then T real-tap products added one at a time in tap order."""
    x = np.asarray(x, np.complex64)
    h = np.asarray(taps, np.float32)
    p = phasor(fc, fs, first + np.arange(len(x), dtype=np.int64)).astype(np.complex64)
    z = np.concatenate([np.zeros(len(h) - 1, np.complex64), (x * p).astype(np.complex64)])
    k = np.arange(0, len(x), decim) + len(h) - 1
    acc = np.zeros(len(k), np.complex64)
    for i in range(len(h)):
        acc = (acc + h[i] * z[k - i]).astype(np.complex64)
    return acc


def f32_composite(x, taps, decim: int, fc: int, fs: int, first: int = 0) -> np.ndarray:
    """Form B with every operation rounded to float32: complex taps rounded once from double, T complex
    products added one at a time, then the rotator product."""
    x = np.asarray(x, np.complex64)
    h = np.asarray(taps, np.float64)
    g = (h * phasor(fc, fs, np.arange(len(h), dtype=np.int64), sign=+1.0)).astype(np.complex64)
    xp = np.concatenate([np.zeros(len(h) - 1, np.complex64), x])
    k = np.arange(0, len(x), decim) + len(h) - 1
    acc = np.zeros(len(k), np.complex64)
    for i in range(len(h)):
        acc = (acc + g[i] * xp[k - i]).astype(np.complex64)
    rot = phasor(fc, fs, first + np.arange(0, len(x), decim, dtype=np.int64)).astype(np.complex64)
    return (acc * rot).astype(np.complex64)
