"""GLONASS FDMA acquisition sweep on the GPU: one code under one Doppler grid per frequency channel in one pass
(gnsship_acq_set_grid_fdma / gnsship_acq_run_fdma), against

* the existing single-grid path run once per channel with set_grid(doppler_center + bias): the same kernels over the
  same table rows, each row reduced by its own workgroup whatever the row count, so every value is compared bitwise;
* the generator's truth;
* the oracle's acquisition_core restatement for one channel, by tests/test_gpu_acq.py's rule (peak position exact
  when the reference itself has no near tie — asserted here, the satellites are strong — and float tolerance on the
  statistic: the FFT implementations differ).
"""
import numpy as np
import pytest

from gnss_sim_receiver_amd import abi, codes, engine, signals
from oracle import oracle as O
from oracle.receiver import calculate_threshold
from test_gpu_acq import TIE

pytestmark = pytest.mark.gpu

FS, N, DMAX, STEP, NB = 4000000, 4000, 5000, 500, 20
CHANNELS = list(range(-3, 4))
PFA = 1e-3  # the acquisition's own decision: pcps_acquisition::calculate_threshold for this pfa, grid and fft size
FIELDS = ("doppler_index", "code_index", "peak", "input_power", "test_statistic", "acq_delay_samples")


def bias(k, signal="1G"):
    return codes.glonass_doppler_bias_hz(signal, k)


def fields(r):
    return tuple(getattr(r, f) for f in FIELDS)


# The scenario (the issue leaves Doppler, delay and grid to the test): the reference's default 500 Hz step for a 1 ms
# dwell, every Doppler on a bin (the neighbouring bins are 500 Hz off: sinc² = 0.41, 3.9 dB down, against 17 dB of
# post-correlation SNR at 47 dB-Hz) and every code start on a whole sample, so "within one sample" leaves a margin of
# two samples (a quarter chip at 7.8 samples per chip).  That the reference itself finds this truth in this noise is
# asserted on the CPU, with the oracle, before the device is looked at.
OCCUPIED = [(-3, -2000.0, 785, 0.4), (0, 1000.0, 2611, 1.1), (2, 3000.0, 3524, 2.9)]  # channel, Doppler, code start [samples], phase


def truth(sat, fs, n):
    """(the generator's Doppler bin, first code start in the buffer [samples])."""
    return int(round((sat.doppler_hz + DMAX) / STEP)), (sat.code_delay_chips / sat.code_freq() * fs) % n


def oracle_channel(sig, fs, n, k, signal="1G"):
    code = codes.glonass_l1_ca_code_gen_complex_sampled(fs)
    w = O.doppler_wipeoff_grid(NB, n, DMAX, STEP, 0, fs, doppler_bias=bias(k, signal))
    rgrid = O.acquisition_grid(sig[:n], code, w)
    spc = int(np.ceil(np.float32(fs) / np.float32(codes.GLONASS_L1_CA_CODE_RATE_CPS)))
    return O.acquisition_statistic(rgrid, DMAX, STEP, 0, True, spc, float(np.float32(np.float32(fs) * np.float32(0.001)))), rgrid


def within_a_sample(code_index, start, n):
    d = abs(code_index - start)
    return min(d, n - d) <= 1.0


@pytest.fixture(scope="module")
def sky():
    sats = []
    for k, d, start, p in OCCUPIED:
        s = signals.Satellite(prn=1, doppler_hz=d, code_delay_chips=0.0, carrier_phase_rad=p, cn0_dbhz=47.0, system="GLO_L1", freq_channel=k)
        s.code_delay_chips = start * s.code_freq() / FS
        sats.append(s)
    sig = signals.generate_if(FS, 2 * N, sats, seed=1602)
    refs = {}
    for s in sats:  # the reference alone finds the truth
        ref, rgrid = oracle_channel(sig, FS, N, s.freq_channel)
        b, start = truth(s, FS, N)
        assert ref.doppler_index == b and within_a_sample(ref.code_index, start, N), (s.freq_channel, ref, start)
        refs[s.freq_channel] = (ref, rgrid)
    return sats, sig, refs


def single_grid_runs(ctx, sig_dwells, channels, fs=FS, signal="1G", want_grid=True, **kw):
    """The existing path: one handle, one set_grid(doppler_center + bias) and one run (per dwell) per channel."""
    n = int(fs / 1000)
    acq = engine.PcpsAcquisition(ctx, fs, kw.pop("fft_size", n), DMAX, STEP, chip_rate=codes.GLONASS_L1_CA_CODE_RATE_CPS, **kw)
    acq.set_local_code(codes.glonass_l1_ca_acquisition_code(fs))
    out = []
    for k in channels:
        acq.set_grid(DMAX, STEP, bias(k, signal))
        for sig in sig_dwells:
            (r,), grid = acq.run(sig, want_grid=want_grid)
        out.append((r, grid[0] if want_grid else None))
    acq.close()
    return out


def assert_channels_equal(res, grid, ref, channels, signal="1G"):
    for g, k in enumerate(channels):
        r, rgrid = ref[g]
        assert fields(res[g]) == fields(r), k
        assert res[g].doppler_hz == r.doppler_hz - bias(k, signal) == -DMAX + STEP * r.doppler_index, k  # reported without the bias
        if rgrid is not None:
            assert np.array_equal(grid[g], rgrid), k


def test_fdma_sweep_equals_one_single_grid_run_per_channel(ctx, sky):
    sats, sig, _ = sky
    acq = engine.glonass_l1_ca_pcps_acquisition(ctx, FS, DMAX, STEP, freq_channels=CHANNELS)
    assert acq.freq_channels == CHANNELS and acq.fdma_channels == 7 and acq.n_bins == NB
    res, grid = acq.run_fdma(sig[:N], want_grid=True)
    assert grid.shape == (7, NB, N)
    ref = single_grid_runs(ctx, [sig[:N]], CHANNELS)
    assert_channels_equal(res, grid, ref, CHANNELS)
    # without a kept grid (the row statistics alone) the decisions are the same
    res2, _ = acq.run_fdma(sig[:N])
    assert [fields(r) for r in res2] == [fields(r) for r in res]
    # the occupied channels report the generator's Doppler bin and code start; the empty ones stay below them
    occupied = {s.freq_channel: s for s in sats}
    for g, k in enumerate(CHANNELS):
        if k in occupied:
            b, start = truth(occupied[k], FS, N)
            assert res[g].doppler_index == b, k
            assert within_a_sample(res[g].code_index, start, N), (k, res[g].code_index, start)
    threshold = calculate_threshold(PFA, N, NB)
    for g, k in enumerate(CHANNELS):  # the block's decision per channel: occupied positive, empty negative
        assert (res[g].test_statistic > threshold) == (k in occupied), (k, res[g].test_statistic, threshold)
    acq.close()


def test_first_vs_second_peak_statistic_per_channel(ctx, sky):
    _, sig, _ = sky
    acq = engine.glonass_l1_ca_pcps_acquisition(ctx, FS, DMAX, STEP, freq_channels=CHANNELS, use_cfar=False)
    res, _ = acq.run_fdma(sig[:N])
    assert_channels_equal(res, None, single_grid_runs(ctx, [sig[:N]], CHANNELS, want_grid=False, use_cfar=False), CHANNELS)
    acq.close()


def test_one_channel_against_the_oracle(ctx, sky):
    sats, sig, refs = sky
    acq = engine.glonass_l1_ca_pcps_acquisition(ctx, FS, DMAX, STEP, freq_channels=CHANNELS)
    res, grid = acq.run_fdma(sig[:N], want_grid=True)
    acq.close()
    for k in (2, -3):
        g = CHANNELS.index(k)
        ref, rgrid = refs[k]
        flat = np.sort(rgrid.ravel())
        assert flat[-1] / flat[-2] > TIE  # the reference alone has no near tie: nothing is skipped
        assert (res[g].doppler_index, res[g].code_index, res[g].doppler_hz) == (ref.doppler_index, ref.code_index, ref.doppler_hz), k
        assert res[g].acq_delay_samples == ref.acq_delay_samples
        np.testing.assert_allclose([res[g].peak, res[g].input_power, res[g].test_statistic], [ref.peak, ref.input_power, ref.test_statistic],
                                   rtol=2e-3)
        assert np.max(np.abs(grid[g] - rgrid)) / rgrid.max() < 1e-5


def test_two_noncoherent_dwells(ctx, sky):
    _, sig, _ = sky
    acq = engine.glonass_l1_ca_pcps_acquisition(ctx, FS, DMAX, STEP, freq_channels=CHANNELS, max_dwells=2)
    first, _ = acq.run_fdma(sig[:N])
    res, grid = acq.run_fdma(sig[N:], want_grid=True)
    ref = single_grid_runs(ctx, [sig[:N], sig[N:]], CHANNELS, max_dwells=2)
    assert_channels_equal(res, grid, ref, CHANNELS)
    assert fields(res[5]) != fields(first[5])  # the second dwell did accumulate
    acq.close()


@pytest.mark.parametrize("mode", ["bit_transition", "zero_padding"])
def test_bit_transition_and_zero_padding(ctx, sky, mode):
    """fft_size 8000 (the single-workgroup transform, where N = 4000 runs the four-step one)."""
    _, sig, _ = sky
    kw = dict(fft_size=2 * N, bit_transition_flag=True) if mode == "bit_transition" else dict(fft_size=2 * N, consumed_samples=N)
    acq = engine.PcpsAcquisition(ctx, FS, kw["fft_size"], DMAX, STEP, chip_rate=codes.GLONASS_L1_CA_CODE_RATE_CPS,
                                 **{a: b for a, b in kw.items() if a != "fft_size"})
    acq.set_local_code(codes.glonass_l1_ca_acquisition_code(FS))
    acq.set_grid_fdma(DMAX, STEP, 0, [bias(k) for k in (-3, 2)])
    res, grid = acq.run_fdma(sig, want_grid=True)
    assert_channels_equal(res, grid, single_grid_runs(ctx, [sig], (-3, 2), **kw), (-3, 2))
    acq.close()


def test_regrid_grows_shrinks_and_returns_to_the_ordinary_grid(ctx, sky):
    _, sig, _ = sky
    acq = engine.glonass_l1_ca_pcps_acquisition(ctx, FS, DMAX, STEP, freq_channels=[0])
    one, _ = acq.run_fdma(sig[:N])
    acq.set_grid_fdma(DMAX, STEP, 0, [bias(k) for k in CHANNELS])  # 20 → 140 rows
    full, full_grid = acq.run_fdma(sig[:N], want_grid=True)
    acq.set_grid_fdma(DMAX, STEP, 0, [bias(2), bias(-3)])  # 140 → 40 rows, another order
    two, two_grid = acq.run_fdma(sig[:N], want_grid=True)
    assert fields(one[0]) == fields(full[3])
    assert [fields(r) for r in two] == [fields(full[5]), fields(full[0])]
    assert np.array_equal(two_grid[0], full_grid[5]) and np.array_equal(two_grid[1], full_grid[0])
    # a doppler_center moves every channel's grid
    acq.set_grid_fdma(DMAX, STEP, 500, [bias(2)])
    (moved,), _ = acq.run_fdma(sig[:N])
    assert (moved.doppler_index, moved.doppler_hz) == (full[5].doppler_index - 1, full[5].doppler_hz)
    # the calls that do not apply to an FDMA grid say so
    for call in (lambda: acq.run(sig[:N]), lambda: acq.set_grid_step2(0.0, 10.0, 4, 1.0)):
        with pytest.raises(abi.GnssHipError) as e:
            call()
        assert e.value.code == abi.E_INVAL
    # no channels, more than 32 channels, more than 4096 rows: refused, and the grid in place stays as it is
    for args in ((DMAX, STEP, 0, []), (DMAX, STEP, 0, [0] * 33), (DMAX, 2, 0, [0])):
        with pytest.raises(abi.GnssHipError) as e:
            acq.set_grid_fdma(*args)
        assert e.value.code == abi.E_INVAL
    (still,), _ = acq.run_fdma(sig[:N])
    assert fields(still) == fields(moved)
    acq.set_grid_fdma(DMAX, STEP, 0, [bias(k % 14 - 7) for k in range(32)])  # the most the call takes: 640 rows
    wide, _ = acq.run_fdma(sig[:N])
    assert [fields(wide[k]) for k in (4, 7, 9)] == [fields(full[0]), fields(full[3]), fields(full[5])]
    # set_grid returns to the ordinary grid: results equal a fresh handle's
    acq.set_grid(DMAX, STEP, 0)
    (back,), back_grid = acq.run(sig[:N], want_grid=True)
    (fresh, fresh_grid), = single_grid_runs(ctx, [sig[:N]], [0])
    assert fields(back) == fields(fresh) == fields(full[3]) and back.doppler_hz == fresh.doppler_hz
    assert np.array_equal(back_grid[0], fresh_grid)
    with pytest.raises(ValueError):
        acq.run_fdma(sig[:N])
    acq.close()


def test_all_fourteen_channels_at_10_msps_l2(ctx):
    fs, n, chans = 10000000, 10000, list(range(-7, 7))
    sats = [signals.Satellite(prn=1, doppler_hz=d, code_delay_chips=c, cn0_dbhz=47.0, system="GLO_L2", freq_channel=k)
            for k, d, c in [(-7, 1500.0, 17.4), (6, -4000.0, 499.1)]]
    sig = signals.generate_if(fs, n, sats, seed=1246)
    acq = engine.glonass_l2_ca_pcps_acquisition(ctx, fs, DMAX, STEP)
    assert acq.freq_channels == chans and acq.conf.fft_size == n
    res, grid = acq.run_fdma(sig, want_grid=True)
    acq.close()
    assert_channels_equal(res, grid, single_grid_runs(ctx, [sig], chans, fs=fs, signal="2G"), chans, signal="2G")
    threshold = calculate_threshold(PFA, n, NB)
    for g, k in enumerate(chans):
        assert (res[g].test_statistic > threshold) == (k in (-7, 6)), (k, res[g].test_statistic, threshold)
