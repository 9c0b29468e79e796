"""The synthetic GPS L5 signal (signals.SYSTEMS["GPS_L5"]): (d·NH10·c_I + j·NH20·c_Q)/√2 per IS-GPS-705 —
the data component L5I in phase, the pilot L5Q in quadrature, 10 code periods per data symbol — and
the existing systems' signals unchanged."""
import hashlib

import numpy as np

from gnss_sim_receiver_amd import codes, signals as S

NH20 = "00000100110101001110"
NH10 = "0000110101"
L = 10230


def pm(s):
    return np.array([1.0 if b == "0" else -1.0 for b in s])


def test_l5_components_quadrature_and_secondary_codes():
    """A noiseless block at one sample per chip, no Doppler, code phase 0: period p correlated against
    L5I gives d·NH10[p mod 10]·A·L/√2 (real) and against L5Q gives j·NH20[p mod 20]·A·L/√2 — the two
    components a quarter cycle apart — over 20 periods (two data symbols)."""
    fs, prn, periods = 10.23e6, 11, 20
    sat = S.Satellite(prn=prn, doppler_hz=0.0, code_delay_chips=0.0, cn0_dbhz=50.0, system="GPS_L5", bits="01")
    assert sat.secondary == NH20 and sat.secondary_data == NH10
    assert np.array_equal(sat.code, codes.gps_l5q_code_gen_float(prn)) and np.array_equal(sat.code_data, codes.gps_l5i_code_gen_float(prn))
    # half a chip early: sample n sits at chip phase n + 0.5, so floor() is safe from rounding
    sat.code_delay_chips = -0.5
    x = S.generate_if(fs, periods * L, [sat], noise=False).astype(np.complex128).reshape(periods, L)
    amp = np.sqrt(2.0 * 10.0 ** 5.0 / fs)
    ci = x @ sat.code_data.astype(np.float64) / (amp * L / np.sqrt(2.0))
    cq = x @ sat.code.astype(np.float64) / (amp * L / np.sqrt(2.0))
    d = np.repeat(pm("01"), 10)[:periods]
    want_i = d * np.tile(pm(NH10), 2)
    want_q = 1j * pm(NH20)
    # the other component leaks only its cross-correlation (|·| < 0.1), so the signs are unambiguous
    assert np.allclose(ci.real, want_i, atol=0.1) and np.all(np.abs(ci.imag) < 0.1)
    assert np.allclose(cq.imag, want_q.imag, atol=0.1) and np.all(np.abs(cq.real) < 0.1)
    # quadrature: pilot / data correlations are ±j apart, period by period
    ratio = cq / ci
    assert np.allclose(ratio.imag, (want_q / want_i).imag, atol=0.25) and np.all(np.abs(ratio.real) < 0.25)


def test_l5_device_generator_matches_numpy():
    sats = [S.Satellite(prn=p, doppler_hz=dd, code_delay_chips=c, cn0_dbhz=60.0, system="GPS_L5", carrier_phase_rad=0.7, bits="0110")
            for p, dd, c in ((3, 1234.5, 100.25), (7, -3210.0, 9017.75))]
    start = 123456
    a = S.generate_if(12.5e6, 60000, sats, noise=False, start=start)
    b = S.generate_if_device(12.5e6, 60000, sats, start=start, device="cpu", noise=False, block=25000).numpy()
    assert np.max(np.abs(a - b)) <= 1e-6 * np.max(np.abs(a))


def test_gps_l1_block_is_unchanged():
    """A GPS L1 block (navigation bits, Doppler ramp, IF, noise) is sample for sample what the generator
    produced before the L5 signal model was added: SHA-256 of the complex64 samples, recorded from the
    parent commit's signals.generate_if."""
    sats = [S.Satellite(prn=7, doppler_hz=1730.0, code_delay_chips=315.6, carrier_phase_rad=0.7, cn0_dbhz=45.0, bits="1000101100110"),
            S.Satellite(prn=19, doppler_hz=-2210.5, code_delay_chips=17.25, cn0_dbhz=47.0, doppler_rate_hz_s=120.0, f_if_hz=20000.0,
                        data_bits=True, bit_seed=3)]
    x = S.generate_if(4e6, 100000, sats, seed=0x15, start=4000000)
    assert x.dtype == np.complex64
    assert hashlib.sha256(x.tobytes()).hexdigest() == GPS_L1_BLOCK_SHA256


GPS_L1_BLOCK_SHA256 = "45594026dc8f72839a5b02dbd4b168e665132a6d72e8a4de5aa0d0b610a28dfd"
