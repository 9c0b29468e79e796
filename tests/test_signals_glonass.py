"""The synthetic generator's GLONASS systems: a satellite sits at its FDMA channel's offset in the IF stream,
its code Doppler follows its own carrier, and despreading with the one C/A code recovers the bits."""
import numpy as np
import pytest

from gnss_sim_receiver_amd import codes, signals

FS = 4e6


def _despread(x, sat, n_periods, first_period=1):
    """Prompt per code period with the truth's code phase and carrier removed."""
    out = np.zeros(n_periods, np.complex128)
    L = sat.code_len
    for i in range(n_periods):
        e = first_period + i
        s0 = int(np.ceil((e * L + sat.code_delay_chips) / sat.code_freq() * FS))
        n = np.arange(s0, s0 + 3990, dtype=np.float64)
        chip = np.floor(sat.chip_phase(n, FS)).astype(np.int64)
        assert np.all(chip // L == e)
        out[i] = np.sum(x[s0:s0 + 3990] * sat.code[chip % L] * np.exp(-1j * sat.carrier_phase(n, FS)))
    return out


@pytest.mark.parametrize("system,dfrq,k,prn", [("GLO_L1", 562500.0, 2, None), ("GLO_L1", 562500.0, -3, None), ("GLO_L2", 437500.0, 1, None),
                                               ("GLO_L1", 562500.0, None, 12)])
def test_spectrum_peak_sits_at_the_channel_offset_plus_doppler(system, dfrq, k, prn):
    dop = 1500.0
    sat = signals.Satellite(prn=prn or 1, doppler_hz=dop, code_delay_chips=100.25, cn0_dbhz=60.0, system=system, freq_channel=k)
    if k is None:  # the table's channel for the PRN
        k = codes.glonass_freq_channel(prn)
        assert sat.freq_channel == k == -1
    assert sat.carrier_hz() == signals.SYSTEMS[system][2] + k * dfrq and sat.if_hz() == k * dfrq
    assert sat.code_freq() == 0.511e6 * (1.0 + dop / sat.carrier_hz())
    n = 40000  # 10 ms: 100 Hz per FFT bin
    x = signals.generate_if(FS, n, [sat], seed=3, noise=False)
    # wiping the code off leaves the carrier alone
    ph = np.floor(sat.chip_phase(np.arange(n, dtype=np.float64), FS)).astype(np.int64)
    spec = np.abs(np.fft.fft(x * sat.code[ph % 511]))
    f = np.fft.fftfreq(n, 1.0 / FS)[int(np.argmax(spec))]
    assert abs(f - (k * dfrq + dop)) < 1.0  # the frequency is a whole bin: the peak is that bin


def test_f_if_adds_to_the_channel_offset_and_other_systems_are_unchanged():
    sat = signals.Satellite(prn=1, doppler_hz=0.0, code_delay_chips=0.0, system="GLO_L1", freq_channel=-1, f_if_hz=250e3)
    assert sat.if_hz() == 250e3 - 562500.0
    gps = signals.Satellite(prn=3, doppler_hz=2000.0, code_delay_chips=5.0, f_if_hz=1e5)
    assert gps.freq_channel is None and gps.if_hz() == 1e5 and gps.carrier_hz() == codes.GPS_L1_FREQ_HZ
    assert gps.code_freq() == 1023000.0 * (1.0 + 2000.0 / codes.GPS_L1_FREQ_HZ)


def test_despreading_recovers_the_meander_half_bits():
    bits = "0110100111"
    sat = signals.Satellite(prn=5, doppler_hz=-2100.0, code_delay_chips=300.5, carrier_phase_rad=0.3, cn0_dbhz=50.0, system="GLO_L1",
                            bits=bits, symbols_per_bit=10)
    assert sat.freq_channel == 1
    n_periods = 100
    x = signals.generate_if(FS, 4000 * (n_periods + 2), [sat], seed=9)
    p = _despread(x, sat, n_periods)
    expect = np.array([1.0 if bits[((1 + i) // 10) % len(bits)] == "0" else -1.0 for i in range(n_periods)])
    # 50 dB-Hz over 1 ms: 20 dB per period — every sign right, and the carrier truly removed (prompt on the real axis)
    assert np.array_equal(np.sign(p.real), expect)
    assert np.all(np.abs(p.imag) < 0.5 * np.abs(p.real))


def test_two_channels_separate_by_frequency_alone():
    """Two satellites with the same code and the same delay on different channels: each despreads to its own bits."""
    a = signals.Satellite(prn=1, doppler_hz=500.0, code_delay_chips=40.0, cn0_dbhz=50.0, system="GLO_L1", freq_channel=2,
                          bits="01", symbols_per_bit=1)
    b = signals.Satellite(prn=2, doppler_hz=500.0, code_delay_chips=40.0, cn0_dbhz=50.0, system="GLO_L1", freq_channel=-3,
                          bits="0011", symbols_per_bit=1)
    x = signals.generate_if(FS, 4000 * 22, [a, b], seed=11)
    pa, pb = _despread(x, a, 20), _despread(x, b, 20)
    assert np.array_equal(np.sign(pa.real), [(-1.0) ** (1 + i) for i in range(20)])
    assert np.array_equal(np.sign(pb.real), [1.0 if ((1 + i) % 4) < 2 else -1.0 for i in range(20)])
