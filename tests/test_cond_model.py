"""Signal conditioner, host side (no GPU): the float64 model of the frequency-translating FIR decimator
(tests/cond_model.py), the honesty of the accuracy contract the device is held to, and the low-pass tap
helper (freq_xlating_fir_filter.cc:99-106).

Accuracy contract: |y − y_ref| ≤ (T + 8)·2⁻²³·Σ_i |h[i]|·|x[kD − i]| — the float32 bound of T rounded
products added one at a time, plus a fixed allowance for the conversion, the mixing product and the
phasor's own rounding.  Two plain float32 formulations (mix-then-FIR; composite taps + rotator) are
checked here to stay inside it, so the bound asks nothing a straightforward implementation cannot give.
"""
import numpy as np
import pytest

import cond_model as M
from gnss_sim_receiver_amd import abi, engine


@pytest.fixture(scope="module")
def x():
    return M.stream("cf32")[1]


@pytest.mark.parametrize("first", M.FIRSTS)
def test_model_forms_agree(x, first):
    """Mix-then-FIR and composite-taps-then-rotate are the same sum: equal to 1e-12 of Σ|h||x|."""
    for T in M.SHAPES_T:
        for D in M.SHAPES_D:
            h = M.windowed_sinc_taps(T, D)
            for fc in M.SHAPES_FC:
                a = M.model_mix_fir(x, h, D, fc, M.FS, first)
                b = M.model_composite(x, h, D, fc, M.FS, first)
                bnd = M.bound(x, h, D)
                assert len(a) == len(b) == len(bnd) == len(x) // D
                assert np.max(np.abs(a - b) / bnd) <= 1e-12, (T, D, fc)


def test_phase_is_exact_far_into_the_stream():
    """frac(fc·n/fs) in integers: periodic in n with period fs, whatever the offset."""
    n = np.arange(0, 5000, dtype=np.int64)
    for fc in M.SHAPES_FC:
        assert np.array_equal(M.phase_frac(fc, M.FS, n), M.phase_frac(fc, M.FS, n + 7000 * M.FS))
    assert M.phase_frac(1_250_000, M.FS, 40) == 0.0 and M.phase_frac(-7_161_000, M.FS, 1) == (M.FS - 7_161_000) / M.FS


@pytest.mark.parametrize("first", M.FIRSTS)
def test_plain_float32_formulations_meet_the_contract(x, first):
    x = x[:2000]  # two windows of the longest filter: the error does not grow with the stream
    worst = 0.0
    for T in M.SHAPES_T:
        for D in M.SHAPES_D:
            h = M.windowed_sinc_taps(T, D)
            for fc in M.SHAPES_FC:
                ref, bnd = M.model(x, h, D, fc, M.FS, first)
                for form in (M.f32_mix_fir, M.f32_composite):
                    r = M.contract_ratio(form(x, h, D, fc, M.FS, first), ref, bnd, T)
                    worst = max(worst, r)
                    assert r <= 1.0, (form.__name__, T, D, fc, r)
    print(f"worst |err| / contract bound over the shape list: {worst:.3f}")


def test_identity_filter_is_exact(x):
    """fc = 0, D = 1, h = [1]: the model returns the input."""
    ref, bnd = M.model(x, [1.0], 1, 0, M.FS)
    assert np.array_equal(ref, x.astype(np.complex128)) and np.array_equal(bnd, np.abs(x.astype(np.complex128)))


def test_cond_lowpass_taps_are_the_adapters_design(built):
    lib = abi.load()
    for fs, d in [(50e6, 5), (16e6, 4), (16e6, 2), (4e6, 1)]:
        bw = (fs / d) / 2
        assert np.array_equal(engine.cond_lowpass_taps(lib, fs, d), engine.firdes_low_pass(lib, 1.0, fs, bw, bw / 10.0))
    assert len(engine.cond_lowpass_taps(lib, 50e6, 5)) == 241
    assert np.array_equal(engine.cond_lowpass_taps(lib, 50e6, 5, 3e6, 1e6), engine.firdes_low_pass(lib, 1.0, 50e6, 3e6, 1e6))
    assert np.array_equal(engine.cond_lowpass_taps(lib, 50e6, 5, 3e6), engine.firdes_low_pass(lib, 1.0, 50e6, 3e6, 3e5))
    assert np.array_equal(engine.cond_lowpass_taps(lib, 50e6, 5, 0.0, 1e6), engine.firdes_low_pass(lib, 1.0, 50e6, 5e6, 1e6))
    for bad in [(0.0, 5, 0.0, 0.0), (50e6, 0, 0.0, 0.0), (50e6, 5, 30e6, 0.0), (50e6, 5, -1.0, 0.0), (50e6, 5, 1e6, -1.0)]:
        with pytest.raises(abi.GnssHipError):
            engine.cond_lowpass_taps(lib, *bad)
    n = abi.ctypes.c_int()
    small = np.zeros(10, np.float32)
    assert lib.gnsship_cond_lowpass_taps(50e6, 5, 0.0, 0.0, abi.fptr(small), 10, abi.ctypes.byref(n)) == abi.E_INVAL and n.value == 241


def test_cond_null_arguments_are_rejected_without_device(built):
    lib = abi.load()
    assert lib.gnsship_cond_create(None, 50e6, None, 1, 1000, None) == abi.E_INVAL
    assert lib.gnsship_cond_run(None, None, 0, 0, 0, None, None, None, None) == abi.E_INVAL
    assert lib.gnsship_cond_reset(None, 0) == abi.E_INVAL
    assert lib.gnsship_cond_samples_in(None, None) == abi.E_INVAL
    assert lib.gnsship_cond_destroy(None) == abi.E_INVAL
