"""The synthetic BeiDou B3I and GPS L2C signals (signals.SYSTEMS["BDS_B3I"], ["GPS_L2C"]): one component each,
despread with their own codes to the configured C/N0 — B3I with NH20 and 20 code periods per navigation bit
(a GEO satellite: no NH, 2 periods per bit), L2C with no secondary code and one symbol per 20 ms code period —
and the existing systems' signals unchanged."""
import hashlib

import numpy as np

from gnss_sim_receiver_amd import codes, signals as S

NH20 = "00000100110101001110"
L = 10230


def pm(s):
    return np.array([1.0 if b == "0" else -1.0 for b in s])


def despread(sat, rate, periods):
    """Noiseless block at one sample per chip, no Doppler, half a chip early (so floor() is safe from
    rounding): period p correlated against the code, in units of the configured amplitude · L."""
    sat.code_delay_chips = -0.5
    x = S.generate_if(rate, periods * L, [sat], noise=False).astype(np.complex128).reshape(periods, L)
    amp = np.sqrt(2.0 * 10.0 ** (sat.cn0_dbhz / 10.0) / rate)
    return x @ sat.code.astype(np.float64) / (amp * L)


def test_b3i_meo_carries_nh20_and_20_periods_per_bit():
    sat = S.Satellite(prn=11, doppler_hz=0.0, code_delay_chips=0.0, cn0_dbhz=50.0, system="BDS_B3I", bits="01")
    assert sat.secondary == NH20 and sat.secondary_data is None and sat.code_data is None
    assert sat.chip_rate == 10.23e6 and sat.code_len == L
    assert np.array_equal(sat.code, codes.beidou_b3i_code_gen_float(11))
    c = despread(sat, 10.23e6, 60)
    want = np.tile(pm(NH20), 3) * np.repeat(pm("010"), 20)
    assert np.allclose(c.real, want, atol=1e-6) and np.all(np.abs(c.imag) < 1e-6)  # amplitude = the configured C/N0's


def test_b3i_geo_has_no_nh_and_2_periods_per_bit():
    sat = S.Satellite(prn=3, doppler_hz=0.0, code_delay_chips=0.0, cn0_dbhz=50.0, system="BDS_B3I", bits="0110", secondary="",
                      symbols_per_bit=2)
    c = despread(sat, 10.23e6, 16)
    assert np.allclose(c.real, np.repeat(np.tile(pm("0110"), 2), 2), atol=1e-6)


def test_l2c_has_no_secondary_and_one_symbol_per_period():
    sat = S.Satellite(prn=7, doppler_hz=0.0, code_delay_chips=0.0, cn0_dbhz=45.0, system="GPS_L2C", bits="0110100")
    assert sat.secondary is None and sat.code_data is None
    assert sat.chip_rate == 0.5115e6 and sat.code_len == L
    assert np.array_equal(sat.code, codes.gps_l2c_m_code_gen_float(7))
    c = despread(sat, 0.5115e6, 14)
    assert np.allclose(c.real, np.tile(pm("0110100"), 2), atol=1e-6) and np.all(np.abs(c.imag) < 1e-6)
    # symbols_per_bit still overrides the default of 1
    sat = S.Satellite(prn=7, doppler_hz=0.0, code_delay_chips=0.0, cn0_dbhz=45.0, system="GPS_L2C", bits="01", symbols_per_bit=3)
    assert np.allclose(despread(sat, 0.5115e6, 6).real, np.repeat(pm("01"), 3), atol=1e-6)


def test_despread_cn0_with_noise():
    """With noise (unit variance per component) the coherent sum over one period has SNR 2·C/N0·T: the mean of
    |correlation|² over the periods gives the configured C/N0 within the estimate's spread."""
    for system, rate, T, cn0, periods in (("BDS_B3I", 10.23e6, 1e-3, 50.0, 200), ("GPS_L2C", 0.5115e6, 20e-3, 45.0, 60)):
        sat = S.Satellite(prn=9, doppler_hz=0.0, code_delay_chips=-0.5, cn0_dbhz=cn0, system=system, carrier_phase_rad=0.3)
        x = S.generate_if(rate, periods * L, [sat], seed=3).astype(np.complex128).reshape(periods, L)
        c = x @ sat.code.astype(np.float64)
        # E|c|² = A²L² + 2L (noise); C/N0 = A²·fs/2
        a2 = (np.mean(np.abs(c) ** 2) - 2.0 * L) / L ** 2
        est = 10.0 * np.log10(a2 * rate / 2.0)
        assert abs(est - cn0) < 0.5, (system, est)


def test_device_generator_matches_numpy():
    sats = [S.Satellite(prn=3, doppler_hz=1234.5, code_delay_chips=100.25, cn0_dbhz=60.0, system="BDS_B3I", carrier_phase_rad=0.7, bits="0110",
                        secondary="", symbols_per_bit=2),
            S.Satellite(prn=7, doppler_hz=-3210.0, code_delay_chips=9017.75, cn0_dbhz=60.0, system="BDS_B3I", carrier_phase_rad=0.7, bits="0110")]
    start = 123456
    a = S.generate_if(12.5e6, 60000, sats, noise=False, start=start)
    b = S.generate_if_device(12.5e6, 60000, sats, start=start, device="cpu", noise=False, block=25000).numpy()
    assert np.max(np.abs(a - b)) <= 1e-6 * np.max(np.abs(a))
    sats = [S.Satellite(prn=5, doppler_hz=410.0, code_delay_chips=77.25, cn0_dbhz=60.0, system="GPS_L2C", carrier_phase_rad=0.2, bits="0110100")]
    a = S.generate_if(1.25e6, 120000, sats, noise=False, start=start)
    b = S.generate_if_device(1.25e6, 120000, sats, start=start, device="cpu", noise=False, block=25000).numpy()
    assert np.max(np.abs(a - b)) <= 1e-6 * np.max(np.abs(a))


def test_existing_blocks_are_unchanged():
    """A GPS L1 block (tests/test_signals_l5.py's, with its recorded SHA-256) and a BeiDou B1I block with
    navigation bits at the default 20 periods per bit are sample for sample what the generator produced
    before the two signals were added (SHA-256 recorded from the parent commit's signals.generate_if)."""
    sats = [S.Satellite(prn=7, doppler_hz=1730.0, code_delay_chips=315.6, carrier_phase_rad=0.7, cn0_dbhz=45.0, bits="1000101100110"),
            S.Satellite(prn=19, doppler_hz=-2210.5, code_delay_chips=17.25, cn0_dbhz=47.0, doppler_rate_hz_s=120.0, f_if_hz=20000.0,
                        data_bits=True, bit_seed=3)]
    x = S.generate_if(4e6, 100000, sats, seed=0x15, start=4000000)
    assert hashlib.sha256(x.tobytes()).hexdigest() == GPS_L1_BLOCK_SHA256
    sats = [S.Satellite(prn=9, doppler_hz=-830.0, code_delay_chips=1015.6, carrier_phase_rad=0.2, cn0_dbhz=46.0, system="BDS", bits="0111",
                        secondary=NH20)]
    x = S.generate_if(4.092e6, 100000, sats, seed=0x16, start=4092000)
    assert hashlib.sha256(x.tobytes()).hexdigest() == BDS_B1I_BLOCK_SHA256


GPS_L1_BLOCK_SHA256 = "45594026dc8f72839a5b02dbd4b168e665132a6d72e8a4de5aa0d0b610a28dfd"
BDS_B1I_BLOCK_SHA256 = "c8545eb5594743220a2439aea69ace31d0dcf8e9118ae94a13936e42c91f0abf"
