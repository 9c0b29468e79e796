"""Shapes and streams shared by the acquisition resampler's coverage tests (tests/test_acq_resampler_cases.py asserts
their conditions on the oracle and the formula alone, tests/test_gpu_acq_resampler_coverage.py runs them on the device).

A shape is (n_taps, D).  gnsship_acq_resampler_create gives a tile opb = min(256, (8192 − n_taps)/D + 1) outputs and the
kernel stages (n_taps + 1)/2 + (opb − 1)·D + n_taps float2 in dynamic LDS; both are restated here so that the table's
annotations are checked and not believed."""
import numpy as np

from gnss_sim_receiver_amd import signals

FORMATS = ("cf32", "ci16", "ci8")
MAX_SAMPLES = 1 << 16

# (n_taps, D, opb, LDS bytes) — the last two as annotations, recomputed by tests/test_acq_resampler_cases.py
SHAPE_TABLE = [
    (1, 1, 256, 2_056),         # no history kernel, hist_cur never flips
    (1, 7, 256, 14_296),        # no history kernel
    (2, 3, 256, 6_144),         # even taps (padded to a float2)
    (4095, 2, 256, 53_224),
    (4096, 1, 256, 51_192),
    (256, 32, 249, 66_560),     # span exactly 8192
    (1001, 27, 256, 67_096),
    (4001, 100, 42, 80_816),
    (4096, 16, 256, 81_792),
    (4096, 17, 241, 81_792),
    (4096, 4096, 2, 81_920),    # the largest
    (4096, 5000, 1, 49_152),
]
SHAPES = [(t, d) for t, d, _, _ in SHAPE_TABLE]
# the automatic designs (acq_resampler_design) whose tiles are cut short and whose LDS passes 64 KiB: (fs_in, opt_acq_fs)
DESIGNS = [(100_000_000, 2e6), (100_000_000, 1e6), (80_000_000, 2e6)]
DESIGN_SHAPES = {(100_000_000, 2e6): (241, 50, 160, 66_496), (100_000_000, 1e6): (481, 100, 78, 67_376), (80_000_000, 2e6): (193, 40, 200, 66_000)}

ALL_FORMATS = {(4096, 4096), (4096, 16), (4096, 5000), (1, 1), (1, 7)}  # the two largest-LDS shapes, opb = 1, n_taps = 1
DEVICE_INPUT = ((1001, 27), "ci16")                                     # also from a device pointer


def opb_of(n_taps, d):
    return min(256, (8192 - n_taps) // d + 1)


def lds_bytes(n_taps, d):
    return 8 * ((n_taps + 1) // 2 + (opb_of(n_taps, d) - 1) * d + n_taps)


def n_outputs(n_taps, d):
    """Outputs of the test stream: two whole tiles and a partial third (never a multiple of opb where opb > 1), at least
    the eleven the call pattern needs; the large decimations, whose tiles hold one or two outputs, have many tiles."""
    opb = opb_of(n_taps, d)
    nk = max(2 * opb + opb // 2 + 1, 11)
    if opb > 1 and nk % opb == 0:
        nk += 1
    assert d * nk <= MAX_SAMPLES
    return nk


def cuts(d, nk):
    """Calls of D, D, 7·D samples (one output, one output, seven) and the rest."""
    return [0, d, 2 * d, 9 * d, nk * d]


def asymmetric_taps(n_taps, seed=None):
    rng = np.random.default_rng(1000 + n_taps if seed is None else seed)
    return (rng.standard_normal(n_taps) / n_taps).astype(np.float32)


def formats_of(index, shape):
    return FORMATS if shape in ALL_FORMATS else (FORMATS[index % 3],)


def stream(fmt, n, seed):
    """(raw, as complex64 exactly as the load converts it)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 6 + 1j * rng.standard_normal(n) * 6).astype(np.complex64)
    if fmt == "cf32":
        return x, x
    raw = signals.to_ibyte(x, 1.0) if fmt == "ci8" else signals.to_ishort(x, 16.0)
    return raw, raw.astype(np.float32).view(np.complex64)


def cases():
    """(id, n_taps, D, fmt) for every asymmetric-tap run."""
    out = []
    for i, (t, d) in enumerate(SHAPES):
        for fmt in formats_of(i, (t, d)):
            out.append((f"T{t}-D{d}-{fmt}", t, d, fmt))
    return out
