"""Every FFT radix, register-point count and layout of the acquisition engine on the GPU (the cases of
tests/acq_fft_model.py: one PRN, two Doppler bins −250 and 0 Hz, fs = 1000·N).

Per case: (a) the handle's layout is the one the case is written for and the model's chooser gives; (b) the
|IFFT|² grid of a noise-only input against the oracle's complex128 grid, RMS(grid − ref)/RMS(ref) within four
times the same figure of the float32 numpy model of that layout on the same inputs (the margin of test_gpu_mit.py:
room for FMA contraction and summation order, which the model does not reproduce; tests/test_acq_fft_model.py shows
on the CPU that one constant off by 2.5e-5 lands beyond four times this bound), and max|grid − ref| < 1e-5·max(ref)
as before; (c) the reductions against the device's OWN grid through the oracle's statistic functions — indices and
delay exactly, the peak bitwise, the sums to the project's rtol 2e-4, first-vs-second to 1 ulp; no near-tie skip,
both sides read the same float32 values.  (d) a planted peak at the delays where the second-peak window, the
column pairs and the column tiles wrap, on one size per layout family.

The device-to-model error ratios measured on the MI355X are tabulated in DESIGN.md ("Acquisition FFT coverage")."""
import numpy as np
import pytest

import acq_fft_model as A
from gnss_sim_receiver_amd import engine, signals
from oracle import oracle as O

pytestmark = pytest.mark.gpu
CASE_IDS = [c.id for c in A.CASES]


def _rel_rms(g, ref):
    g, ref = g.astype(np.float64), ref.astype(np.float64)
    return float(np.sqrt(np.mean((g - ref) ** 2) / np.mean(ref ** 2)))


def _modes(n):
    """CFAR and first-vs-second; below 30 points CFAR only (the ±samples_per_chip window is most of the row)."""
    return (True, False) if n >= 30 else (True,)


def _open(ctx, monkeypatch, case, cfar, code):
    for k, v in case.env.items():  # read at create
        monkeypatch.setenv(k, v)
    acq = engine.PcpsAcquisition(ctx, 1000 * case.n, case.n, A.DOPPLER_MAX, A.DOPPLER_STEP, 0, cfar)
    try:
        assert acq.n_bins == 2
        assert acq.layout == case.layout == A.choose_layout(case.n, case.force, case.huge_p)  # (a)
        acq.set_local_code(code)
    except BaseException:
        acq.close()
        raise
    return acq


def _check_reductions(res, g, n, cfar, label):
    """(c): the result against the oracle's statistic of the device's own grid g[2, n]."""
    assert int(np.count_nonzero(g == g.max())) == 1, label  # the device grid's maximum is unique
    st = O.acquisition_statistic(g, A.DOPPLER_MAX, A.DOPPLER_STEP, 0, cfar, A.samples_per_chip(n), A.samples_per_code(n))
    assert (res.doppler_index, res.code_index, res.doppler_hz) == (st.doppler_index, st.code_index, st.doppler_hz), label
    assert res.acq_delay_samples == st.acq_delay_samples, label
    assert np.float32(res.peak).tobytes() == g[res.doppler_index, res.code_index].tobytes(), label
    if cfar:
        np.testing.assert_allclose([res.input_power, res.test_statistic], [st.input_power, st.test_statistic], rtol=2e-4, err_msg=str(label))
    else:
        assert np.float32(res.input_power).tobytes() == np.float32(st.input_power).tobytes(), label  # the second peak, a grid value
        want = np.float32(res.peak) / np.float32(st.input_power)
        assert abs(np.float32(res.test_statistic) - want) <= np.spacing(want), (label, res.test_statistic, want)


@pytest.mark.parametrize("case", A.CASES, ids=CASE_IDS)
def test_layout_grid_and_reductions(ctx, monkeypatch, case):
    n = case.n
    r = A.reference(n)
    base = _rel_rms(A.grid(r.sig, r.code, r.wipe, case.layout, np.complex64), r.ref)
    for cfar in _modes(n):
        acq = _open(ctx, monkeypatch, case, cfar, r.code)
        try:
            (res,), grid = acq.run(r.sig, want_grid=True)
            (res_nogrid,), _ = acq.run(r.sig)  # the huge layout then keeps no |y|² rows and recomputes the tiles it rescans
        finally:
            acq.close()
        assert bytes(res_nogrid) == bytes(res), (case.id, cfar)
        g = grid[0]
        err, peak_err = _rel_rms(g, r.ref), float(np.max(np.abs(g.astype(np.float64) - r.ref)) / r.ref.max())
        print(f"\nacq-fft-coverage {case.id} {'cfar' if cfar else 'first-vs-second'}: device {err:.3e} model {base:.3e} "
              f"ratio {err / base:.2f} max-err/max {peak_err:.2e}")
        assert err <= 4.0 * base, (case.id, err, base)                   # (b)
        assert peak_err < 1e-5, (case.id, peak_err)
        _check_reductions(res, g, n, cfar, (case.id, cfar))               # (c)
        assert (res.doppler_index, res.code_index) == np.unravel_index(np.argmax(r.ref), r.ref.shape), case.id


@pytest.mark.parametrize("case", [c for c in A.CASES if c.planted], ids=[c.id for c in A.CASES if c.planted])
def test_planted_peak_at_the_wrapping_delays(ctx, monkeypatch, case):
    """(d): sig = A·roll(code, d) + noise, the peak about 20× over the noise cells; (c) at every d."""
    n = case.n
    delays = A.planted_delays(case, A.samples_per_chip(n))
    assert {0, n - 1} <= set(delays)  # the second-peak window wraps at both ends
    for cfar in (True, False):
        acq = _open(ctx, monkeypatch, case, cfar, A.reference(n, delays[0]).code)
        try:
            for d in delays:
                r = A.reference(n, d)
                (res,), grid = acq.run(r.sig, want_grid=True)
                _check_reductions(res, grid[0], n, cfar, (case.id, cfar, d))
                assert (res.doppler_index, res.code_index) == np.unravel_index(np.argmax(r.ref), r.ref.shape), (case.id, d)
                assert res.code_index == d
                assert np.max(np.abs(grid[0].astype(np.float64) - r.ref)) / r.ref.max() < 1e-5, (case.id, d)
        finally:
            acq.close()


@pytest.mark.parametrize("cid", ["270-big", "480-huge8"])
def test_ci16_input_on_other_register_point_counts(ctx, monkeypatch, cid):
    """16-bit integer input through the column kernels of a four-step P outside {16, 25, 32} (18) and a huge P
    outside {4, 5, 10} (8): (bin, index) against the oracle on the converted samples."""
    case = next(c for c in A.CASES if c.id == cid)
    n, d = case.n, case.layout.row_len + 1
    sig, code = A.planted_inputs(n, d)
    raw = signals.to_ishort(sig, scale=1024.0)
    acq = _open(ctx, monkeypatch, case, True, code)
    try:
        (res,), _ = acq.run(raw)
    finally:
        acq.close()
    ref, rgrid = O.pcps_acquisition_core(raw.astype(np.float32).view(np.complex64), code, 1000 * n, A.DOPPLER_MAX, A.DOPPLER_STEP, 0, True)
    flat = np.sort(rgrid.ravel().astype(np.float64))
    assert (flat[-1] - flat[-2]) / flat[-1] > 1e-3  # a unique maximum: no near-tie
    assert (res.doppler_index, res.code_index) == (ref.doppler_index, ref.code_index) and ref.code_index == d
    np.testing.assert_allclose(res.test_statistic, ref.test_statistic, rtol=2e-3)
