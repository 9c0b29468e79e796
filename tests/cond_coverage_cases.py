"""Cases shared by the signal conditioner's coverage tests (tests/test_cond_coverage_cases.py asserts their conditions
on the model alone, tests/test_gpu_cond_coverage.py runs them on the device): asymmetric taps, the extremes of the
sample rate, decimations next to the tile length, four bands of unlike length in one handle."""
import numpy as np

import cond_model as M

FC = -7_161_000

# ---- asymmetric taps ----
ASYM_T = (2, 64, 1025, 1026, 4096)
ASYM_D = (1, 5)
ASYM_FORMATS = ("cf32", "ci8")


def asymmetric_taps(n_taps, seed=None):
    """Seeded normal values scaled to unit absolute sum, float32: no symmetry for a mirrored window to hide behind."""
    rng = np.random.default_rng(2000 + n_taps if seed is None else seed)
    r = rng.standard_normal(n_taps)
    return (r / np.abs(r).sum()).astype(np.float32)


# ---- rate extremes ----
FS_MAX = 2**31 - 1
RATE_T = (64, 1026)
RATE_D = 2


def rate_fcs(fs=FS_MAX):
    return (1, fs - 1, -(fs - 1), fs + 12345)


def rate_firsts(n):
    return (0, 2**31 + 12345, 2**62 - 1 - n)


# ---- decimation against the tile ----
def tile_of(t_max):
    """The tile length of gnsship_cond_create: the span (8 samples per lane of 256, or 32 where the history passes half
    of that) less the history of max T − 1 samples."""
    n_hist = t_max - 1
    return (2048 if n_hist <= 1024 else 8192) - n_hist


def tile_decimations(t):
    """D one below, at and one above the tile, and about one and a half tiles (3000 for the 1985-sample tile of T = 64);
    the long tile also with D = 3000, several outputs to a tile but never a whole number."""
    tile = tile_of(t)
    if t == 64:
        assert tile == 1985
        return (1984, 1985, 1986, 3000)
    return (tile - 1, tile, tile + 1, 3000, tile * 3 // 2)


def outputs_per_tile(t, d, n):
    tile = tile_of(t)
    k = np.arange(0, n, d)
    return np.bincount(k // tile, minlength=-(-n // tile))


# ---- four bands of unlike length ----
FOUR_BANDS = ((0, 1, 1), (1_250_000, 2, 64), (FC, 5, 1025), (12_345_678, 4, 4096))  # (fc, D, T)
FOUR_CUTS = (0, 20, 140, 3000, 3020, M.N_IN)


def four_bands():
    return [(fc, d, asymmetric_taps(t)) for fc, d, t in FOUR_BANDS]


_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def stream(fmt, n=M.N_IN, seed=20):
    return cached(("stream", fmt, n, seed), lambda: M.stream(fmt, n, seed))
