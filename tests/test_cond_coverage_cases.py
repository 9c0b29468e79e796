"""The conditions the conditioner's coverage cases rely on (tests/cond_coverage_cases.py), on the model alone, no GPU:
with them the GPU tests of tests/test_gpu_cond_coverage.py cannot pass vacuously."""
import numpy as np
import pytest

import cond_coverage_cases as C
import cond_model as M


@pytest.mark.parametrize("T", C.ASYM_T)
@pytest.mark.parametrize("fmt", C.ASYM_FORMATS)
def test_reversed_taps_violate_the_bound(fmt, T):
    """The model fed the reversed taps, rounded to float32, misses the contract bound of the right taps on the test
    stream — by a wide margin, so a mirrored tap window cannot pass the GPU test."""
    _, x = C.stream(fmt)
    h = C.asymmetric_taps(T)
    assert h.dtype == np.float32 and not np.array_equal(h, h[::-1])
    assert abs(float(np.abs(h.astype(np.float64)).sum()) - 1.0) < 1e-5
    for D in C.ASYM_D:
        y_ref, bnd = M.model(x, h, D, C.FC, M.FS)
        wrong = M.model_mix_fir(x, h[::-1], D, C.FC, M.FS).astype(np.complex64)
        right = y_ref.astype(np.complex64)
        assert M.contract_ratio(right, y_ref, bnd, T) <= 1.0
        assert M.contract_ratio(wrong, y_ref, bnd, T) > 100.0
        # an off-by-one window (taps shifted by one sample) too
        shifted = M.model_mix_fir(x, np.concatenate([h[1:], h[:1]]), D, C.FC, M.FS).astype(np.complex64)
        assert M.contract_ratio(shifted, y_ref, bnd, T) > 100.0


def test_rate_extremes_reach_the_limits_of_the_phase_arithmetic():
    fs, n = C.FS_MAX, M.N_IN
    assert fs == 2**31 - 1
    fcs, firsts = C.rate_fcs(), C.rate_firsts(n)
    assert fcs == (1, fs - 1, -(fs - 1), fs + 12345) and firsts == (0, 2**31 + 12345, 2**62 - 1 - n)
    assert max(firsts) + n - 1 < 2**62 and max(firsts) <= (2**63 - 1) // 2      # what gnsship_cond_reset admits
    # the residues the kernel multiplies: fc mod fs up to fs − 1, n mod fs up to fs − 1 on the last first sample
    assert {fc % fs for fc in fcs} == {1, fs - 1, 12345}
    top = (firsts[2] + np.arange(n, dtype=np.int64)) % fs
    assert top.max() == fs - 1 and top.min() == fs - n
    assert (fs - 1) * int(top.max()) > 2**61                                    # the product nearest 2^64 that can occur
    step = ((fs - 1) * 256) % fs
    assert step + (fs - 1) > 2**31                                              # rr + step_mod passes 2^31, stays below 2^32
    assert step + (fs - 1) < 2**32
    # the first sample matters: for fc = fs + 12345 the model at another first sample misses the bound
    _, x = C.stream("cf32")
    for T in C.RATE_T:
        h = C.asymmetric_taps(T)
        y_ref, bnd = M.model(x, h, C.RATE_D, fcs[3], fs, firsts[0])
        for first in firsts[1:]:
            other = M.model_mix_fir(x, h, C.RATE_D, fcs[3], fs, first).astype(np.complex64)
            assert M.contract_ratio(other, y_ref, bnd, T) > 100.0
    # fc = ±(fs − 1) is ∓1 Hz: its phase is too slow to tell a sign or a first sample by, it is there for the size of the
    # products alone; fc = fs + 12345 carries the checks above
    # fs = 1: no phase at all
    assert np.all(M.phase_frac(5, 1, 12345 + np.arange(n)) == 0.0)
    assert np.all(M.phasor(5, 1, 12345 + np.arange(n)) == 1.0)


@pytest.mark.parametrize("T", [64, 1026])
def test_decimations_sit_on_both_sides_of_the_tile(T):
    tile = C.tile_of(T)
    assert tile == (1985 if T == 64 else 7167)
    ds = C.tile_decimations(T)
    assert {tile - 1, tile, tile + 1} <= set(ds) and 3000 in ds
    empty = one = several = False
    for D in ds:
        n = 4 * D
        assert n <= 1 << 16
        per = C.outputs_per_tile(T, D, n)
        assert per.sum() == 4 and len(per) == -(-n // tile)
        empty |= bool((per == 0).any())
        one |= bool((per == 1).any())
        several |= bool((per > 1).any())
    assert empty and one and several
    # an output on a tile's first sample past tile 0 (D = tile) and on a tile's last (D = tile − 1, k = 1)
    assert (1 * tile) % tile == 0 and (tile - 1) % tile == tile - 1


def test_four_bands_differ_in_length_rate_and_tile():
    bands = C.four_bands()
    assert [len(h) for _, _, h in bands] == [1, 64, 1025, 4096]
    assert len({d for _, d, _ in bands}) == 4 and len({fc for fc, _, _ in bands}) == 4
    tiles = [C.tile_of(len(h)) for _, _, h in bands]
    assert C.tile_of(4096) == 8192 - 4095 and tiles[:3] == [2048, 1985, 1024] and len(set(tiles)) == 4
    lcm = int(np.lcm.reduce([d for _, d, _ in bands]))
    assert all(c % lcm == 0 for c in C.FOUR_CUTS) and C.FOUR_CUTS[-1] == M.N_IN
    lens = np.diff(C.FOUR_CUTS)
    assert lens.min() < 64 and lens.max() > C.tile_of(1)      # a call shorter than three histories, one of several tiles
