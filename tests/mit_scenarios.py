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



# ---- coverage scenarios (tests/test_gpu_mit_coverage.py; conditions asserted in tests/test_mit_model.py) ----

# Segment lengths beside the strides of the kernels: no whole group of 8 in mit_chain (2), whole groups and a remainder
# (13, 255, 257), one below and one above the 256-lane strides of the DFT and the LDS loads (255, 257).
COV_LENGTHS = (2, 13, 255, 257)
COV_N_COEFF = 3


# Lengths 2 and 13: the adapters' pfa = 0.001.  Lengths 255 and 257: as at 1024 the pfa threshold (614, 619) lies
# below noise alone — the model's E/noise is 565 to 1060 on noise, 3200 and more where the tone covers part of a
# segment, 11 800 and more where it covers all of it — so 2000 lets the tone decide.
def cov_notch_thres(length):
    return 2000.0 if length >= 255 else thres_pfa(0.001, length)


# seeds at which every detection segment has E/(noise·thres) outside [1 − 1e-3, 1 + 1e-3], picked as NOTCH_SEEDS was:
# the first from 101 on (tests/test_mit_model.py::test_coverage_lengths_keep_clear_of_the_threshold)
COV_NOTCH_SEEDS = {(M.NOTCH, 2): 101, (M.NOTCH, 13): 101, (M.NOTCH, 255): 101, (M.NOTCH, 257): 101,
                   (M.NOTCH_LITE, 2): 101, (M.NOTCH_LITE, 13): 101, (M.NOTCH_LITE, 255): 101, (M.NOTCH_LITE, 257): 101}


def run_cut_sample(length, n):
    """The cut of the two-run tests: RUN_CUT_SEG on the (compressed) pattern of cw_gated, inside a tone span."""
    scale = min(1.0, (n / length) / 300.0)
    return int(RUN_CUT_SEG * scale * length)


def cov_length_case(kind, length):
    """(stream, threshold, model after one whole run, model output) for a coverage length."""
    def make():
        if kind == M.PULSE_BLANKING:
            x, th = pulsed(length), thres_pfa(0.04, length)
        else:
            x, th = cw_gated(length, COV_NOTCH_SEEDS[(kind, length)]), cov_notch_thres(length)
        m = M.Model(kind, th, length, N_EST, N_RESET, p_c=0.9, n_coeff=COV_N_COEFF)
        y = m.run(x)
        return x, th, m, y
    return cached(("cov-length", kind, length), make)


COV_CHAIN_LENGTHS = (13, 257)


def cov_chain_case(length, p_c, chunk_samples, warmup_samples):
    """cw_continuous through the notch at a coverage length, the speculative form emulated."""
    def make():
        x = cw_continuous(CHAIN_N, CHAIN_SEED)
        th = cov_notch_thres(length)
        m = M.Model(M.NOTCH, th, length, N_EST, 5000000, p_c=p_c, chunk_samples=chunk_samples, warmup_samples=warmup_samples)
        y = m.run(x)
        return x, th, m, y
    return cached(("cov-chain", length, p_c, chunk_samples, warmup_samples), make)


def segs_to_samples(kind, seg_counts):
    """Run lengths in samples that emit the given numbers of segments run after run: the notch emits a segment one
    sample late (its one-sample advance), so its first run takes one sample more."""
    out = [c * LONG_LENGTH for c in seg_counts]
    if kind == M.NOTCH and out:
        out[0] += 1
    return out


def gated_by_segment(kind, on_segments, seed=LONG_SEED, amp=8.0):
    """8192 segments of 8 samples, the tone on over exactly the block's segments named by the boolean array: the notch's
    segment s holds input samples s·8 + 1 .. s·8 + 8, the other blocks' s·8 .. s·8 + 7."""
    x = noise(LONG_N, seed)
    t = np.arange(LONG_N)
    shift = 1 if kind == M.NOTCH else 0
    seg = (t - shift) // LONG_LENGTH
    on = np.where(seg >= 0, np.asarray(on_segments, bool)[np.clip(seg, 0, None)], False)
    return (x + on * amp * np.exp(2j * np.pi * 0.0731 * t)).astype(np.complex64)


# Runs of filtered segments against the scan's tiles of 1024: one tile exactly; across an edge; a single segment last
# in a tile ("a") or first in a tile ("b": adjacent single segments would be one run, so there are two streams); one
# longer than two tiles, so that tiles 5 and 6 lie wholly inside it.
EDGE_RUNS = {"a": ((1024, 2048), (3071, 3073), (4095, 4096), (5000, 7500)),
             "b": ((1024, 2048), (3071, 3073), (4096, 4097), (5000, 7500))}
EDGE_CUT_SEGS = (1023, 1025, 2049)


def edge_on_segments(which):
    on = np.zeros(LONG_N // LONG_LENGTH, bool)
    for a, b in EDGE_RUNS[which]:
        on[a:b] = True
    return on


def edge_case(kind, n_coeff, which):
    def make():
        x = gated_by_segment(kind, edge_on_segments(which))
        th = 200.0  # as long_case: between noise alone and the tone
        m = M.Model(kind, th, LONG_LENGTH, N_EST, 5000000, p_c=0.9, n_coeff=n_coeff)
        y = m.run(x)
        return x, th, m, y
    return cached(("edge", kind, n_coeff, which), make)


# A reset among the tiles: the gating of long_gated with n_segments_reset = 3000.  RESET_CUT_SEGS: run 2 starts with
# n_segments = 2001 = n_reset − 1000 + 1 (walked), run 3 starts at segment 3001, where the reset falls, run 4 starts
# with n_segments = 2000 = n_reset − 1000 (decided at once): the two sides of the scan's decision.
RESET_N_RESET = 3000
RESET_CUT_SEGS = (2001, 1000, 2000, 1000)


def reset_on_segments():
    return (np.arange(LONG_N // LONG_LENGTH) % 1000) >= 300


def reset_case(kind, n_coeff=COV_N_COEFF):
    def make():
        x = gated_by_segment(kind, reset_on_segments())
        th = 200.0
        m = M.Model(kind, th, LONG_LENGTH, N_EST, RESET_N_RESET, p_c=0.9, n_coeff=n_coeff)
        y = m.run(x)
        return x, th, m, y
    return cached(("reset", kind, n_coeff), make)


ZERO_LENGTH = 32


def leading_zeros_case(kind):
    """3·n_est all-zero segments, then the content of the length-32 scenarios.  Pulse blanking's estimate is 0 and the
    ratios after it are 0/0 and x/0; the notches' is the 1e-20 of the power spectrum."""
    def make():
        L = ZERO_LENGTH
        if kind == M.PULSE_BLANKING:
            tail, th = pulsed(L), thres_pfa(0.04, L)
        else:
            tail, th = cw_gated(L, NOTCH_SEEDS[(kind, L)]), notch_thres(L)
        x = np.concatenate([np.zeros(3 * N_EST * L, np.complex64), tail])
        m = M.Model(kind, th, L, N_EST, N_RESET, p_c=0.9, n_coeff=COV_N_COEFF)
        y = m.run(x)
        return x, th, m, y
    return cached(("zeros", kind), make)


def cov_notch_models():
    """Every new notch scenario's model, for the estimate's tolerance (four times the worst est_err)."""
    out = [cov_length_case(k, L)[2] for k in (M.NOTCH, M.NOTCH_LITE) for L in COV_LENGTHS]
    out += [edge_case(k, COV_N_COEFF, w)[2] for k in (M.NOTCH, M.NOTCH_LITE) for w in EDGE_RUNS]
    out += [reset_case(k)[2] for k in (M.NOTCH, M.NOTCH_LITE)]
    out += [leading_zeros_case(k)[2] for k in (M.NOTCH, M.NOTCH_LITE)]
    return out
