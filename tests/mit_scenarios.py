"""Streams and configurations shared by the interference-mitigation tests (tests/test_mit_model.py asserts their
conditions on the model alone, tests/test_gpu_mit.py runs them on the device).  Every stream stays at or below
2^16 samples.  Model results are computed once per scenario and shared."""
import numpy as np
from scipy.stats import chi2

import mit_model as M

N_EST, N_RESET = 8, 40
LENGTHS = (5, 32, 1024)


def thres_pfa(pfa, length):
    """chi²(2·length) upper pfa quantile, one rounding to float32."""
    return float(np.float32(chi2.isf(pfa, 2 * length)))


def n_samples(length):
    return min(1 << 16, 300 * length + 3)


def noise(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def pulsed(length, seed=11):
    """Unit-variance noise with DME-like pulses: bursts of 12σ, a few segments apart, of 1..2·length samples."""
    n = n_samples(length)
    x = noise(n, seed)
    rng = np.random.default_rng(seed + 1)
    pos = 9 * length
    while pos < n:
        w = int(rng.integers(1, 2 * length + 1))
        x[pos:pos + w] += np.complex64(12.0) * np.exp(1j * rng.uniform(0, 2 * np.pi, len(x[pos:pos + w]))).astype(np.complex64)
        pos += int(rng.integers(2, 30)) * length + int(rng.integers(0, length))
    return x


# tone on / off in segments (fractions: mid-segment switches): on inside the first estimation window, across the
# cut of RUN_CUT_SEG, and a long last one
TONE_SPANS = ((3.5, 20.25), (45.3, 60.0), (100.0, 130.5), (180.2, 181.1), (220.0, 290.7))
RUN_CUT_SEG = 110.4


def cw_gated(length, seed, amp=6.0, f=0.0731):
    """Unit-variance noise plus a CW tone of `amp`σ switched on and off mid-stream (TONE_SPANS)."""
    n = n_samples(length)
    x = noise(n, seed)
    t = np.arange(n)
    tone = (amp * np.exp(2j * np.pi * f * t)).astype(np.complex64)
    nseg = n / length
    scale = min(1.0, nseg / 300.0)  # the 1024-sample segments have 64 of them: the same pattern, compressed
    for a, b in TONE_SPANS:
        i0, i1 = int(a * scale * length), int(b * scale * length)
        x[i0:i1] += tone[i0:i1]
    return x


def cw_continuous(n, seed, amp=10.0, f=0.0731):
    """Noise plus a CW tone from the first sample on: one unbroken filtered run once the estimate is made."""
    return (noise(n, seed) + amp * np.exp(2j * np.pi * f * np.arange(n))).astype(np.complex64)


# Notch thresholds.  Lengths 5 and 32: the adapters' pfa = 0.001.  Length 1024: the estimate sits 2.5 dB under
# the noise power (the mean of dB values), so noise alone gives E/noise ≈ 2·1024/0.56 ≈ 3650 against a pfa
# threshold of 2251 and every segment would filter; 4500 lets the tone decide.
def notch_thres(length):
    return 4500.0 if length == 1024 else thres_pfa(0.001, length)


# seeds at which every detection segment has E/(noise·thres) outside [1 − 1e-3, 1 + 1e-3]
# (tests/test_mit_model.py::test_notch_scenarios_keep_clear_of_the_threshold)
NOTCH_SEEDS = {(M.NOTCH, 5): 101, (M.NOTCH, 32): 102, (M.NOTCH, 1024): 101,
               (M.NOTCH_LITE, 5): 101, (M.NOTCH_LITE, 32): 102, (M.NOTCH_LITE, 1024): 101}
CHAIN_SEED = 7
CHAIN_N = 1 << 16

_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def notch_case(kind, length, n_coeff=1):
    """(stream, threshold, model after one whole run, model output)."""
    def make():
        x = cw_gated(length, NOTCH_SEEDS[(kind, length)])
        th = notch_thres(length)
        m = M.Model(kind, th, length, N_EST, N_RESET, p_c=0.9, n_coeff=n_coeff)
        y = m.run(x)
        return x, th, m, y
    return cached(("notch", kind, length, n_coeff), make)


def pulse_case(length):
    def make():
        x = pulsed(length)
        th = thres_pfa(0.04, length)
        m = M.Model(M.PULSE_BLANKING, th, length, N_EST, N_RESET)
        y = m.run(x)
        return x, th, m, y
    return cached(("pb", length), make)


def chain_case(p_c, chunk_samples, warmup_samples):
    """The continuous-CW stream through the notch (length 32) with the speculative form emulated."""
    def make():
        x = cw_continuous(CHAIN_N, CHAIN_SEED)
        th = thres_pfa(0.001, 32)
        m = M.Model(M.NOTCH, th, 32, N_EST, 5000000, p_c=p_c, chunk_samples=chunk_samples, warmup_samples=warmup_samples)
        y = m.run(x)
        return x, th, m, y
    return cached(("chain", p_c, chunk_samples, warmup_samples), make)


def chain_geometry(p_c, length=32):
    """chunk_samples, warmup_samples as mit_filter.hip derives them (gnsship_mit_create): twice the decay to
    2^-24 plus a segment, whole segments, capped at 4096 samples; chunks of at least 2048 samples and four
    warm-ups."""
    warm = 4096
    if abs(p_c) < 1.0:
        n0 = np.ceil(24.0 * np.log(2.0) / -np.log(abs(p_c))) if p_c != 0 else 1.0
        if 2.0 * n0 < 4096:
            warm = int(2.0 * n0)
    warm_segs = (warm + length - 1) // length + 1
    chunk_segs = max((2048 + length - 1) // length, 4 * warm_segs)
    return chunk_segs * length, warm_segs * length


LONG_LENGTH, LONG_N, LONG_SEED = 8, 1 << 16, 31


def long_gated(seed=LONG_SEED):
    """8192 segments of 8 samples, the tone off for 300 and on for 700 of every 1000 segments: with n_segments_reset out of reach the
    scan's tiles past the first take the path that decides a whole tile at once (mit_scan_kernel)."""
    x = noise(LONG_N, seed)
    t = np.arange(LONG_N)
    on = (t // LONG_LENGTH) % 1000 >= 300  # off over the estimation window
    return (x + on * 8.0 * np.exp(2j * np.pi * 0.0731 * t)).astype(np.complex64)


def long_case(kind, n_coeff):
    def make():
        x = long_gated()
        th = 200.0  # between noise alone (E/noise about 30) and the tone (about 900): the gating decides
        m = M.Model(kind, th, LONG_LENGTH, N_EST, 5000000, p_c=0.9, n_coeff=n_coeff)
        y = m.run(x)
        return x, th, m, y
    return cached(("long", kind, n_coeff), make)

