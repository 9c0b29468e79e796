"""The GLONASS L1 / L2 C/A tracking loop on the device (GNSSHIP_SYS_GLO_L1CA / _L2CA: trk_glo_loop.h on trk_persist.hip's
generic serial pipeline) against tests/glonass_model.py, the block restated in numpy: every field of every epoch
record equal (test_gpu_trk.compare_exact).  Every scenario is first checked on the CPU: the model alone holds lock
(or, for the noise case, loses it), before the device is compared.  Each test asserts the persistent engine ran."""
import numpy as np
import pytest

from gnss_sim_receiver_amd import abi, codes, engine, signals
from oracle import trk as T

import glonass_model as M
import trk_scenarios as S
from test_gpu_trk import compare_exact, dev_conf

pytestmark = pytest.mark.gpu
FS, VL, EPOCHS, CODE_ID = 4000000, 4000, 150, 30
PRN_OF_CHANNEL = {2: 24, -3: 18, 1: 1, 0: 11, 5: 3, -7: 10}
SYSTEM = {"1G": ("GLO_L1", abi.SYS_GLO_L1CA, engine.glonass_l1_ca_trk_conf), "2G": ("GLO_L2", abi.SYS_GLO_L2CA, engine.glonass_l2_ca_trk_conf)}


def satellite(signal, k, doppler=1830.0, delay=207.3, phase=0.9, cn0=50.0, **kw):
    sat = signals.Satellite(prn=PRN_OF_CHANNEL[k], doppler_hz=doppler, code_delay_chips=delay, carrier_phase_rad=phase, cn0_dbhz=cn0,
                            system=SYSTEM[signal][0], bits="0100111010110001", symbols_per_bit=10, **kw)
    assert sat.freq_channel == k == codes.glonass_freq_channel(sat.prn)
    return sat


def acquisition(sat, stamp=0, first=0):
    """start's arguments: the truth, 0.3 samples and 25 Hz off."""
    return signals.acq_delay_samples(sat, FS, stamp, first) + 0.3, sat.doppler_hz + 25.0, stamp, first


def model_run(signal, sat, x, epochs=EPOCHS, start=None, **kw):
    m = M.GlonassTracking(signal, FS, sat.freq_channel, prn=sat.prn, **kw)
    m.start_tracking(*(start or acquisition(sat)))
    ref = m.run(x, 0, epochs)
    return m, ref


def holds_lock(m, ref, epochs=EPOCHS):
    return len(ref) == epochs and m.enable_tracking and not m.events and m.carrier_lock_fail_counter == 0


def device_run(ctx, signal, sat, x, epochs=EPOCHS, start=None, dump=False, **kw):
    ctx.set_code(CODE_ID, codes.glonass_l1_ca_code_gen_float())
    trk = engine.DllPllVemlTracking(ctx, SYSTEM[signal][2](FS, **kw), 1)
    delay, dop, stamp, first = start or acquisition(sat)
    trk.start(0, CODE_ID, delay, dop, stamp, first, prn=sat.prn)
    out = trk.run(x, 0, epochs, dump=dump)
    assert trk.last_engine() == abi.TRK_ENGINE_PERSIST
    state = trk.channel_state(0)
    trk.close()
    return out, state


@pytest.mark.parametrize("signal,k", [("1G", 2), ("1G", -3), ("2G", 1)])
def test_channel_equals_the_model(ctx, signal, k):
    """150 epochs: thirteen lock tests and the carrier-phase initialisation at the first of them."""
    sat = satellite(signal, k, doppler=1830.0 if k > 0 else -2410.0)
    x = signals.generate_if(FS, (EPOCHS + 3) * VL, [sat], seed=100 + k)
    m, ref = model_run(signal, sat, x)
    assert holds_lock(m, ref) and np.count_nonzero(np.diff(ref["cn0_db_hz"])) >= 7
    (rec, done), (state, nxt) = device_run(ctx, signal, sat, x)
    compare_exact(rec[:, 0], ref, f"{signal} k={k}")
    assert done == EPOCHS and state == 4 and nxt == m.sample_counter
    assert np.all(rec[:, 0]["state"] == 4) and np.all(rec[:, 0]["flags"] == 9)


@pytest.mark.parametrize("fmt", ["ci16", "ci8"])
def test_integer_input(ctx, fmt):
    sat = satellite("1G", 2)
    xf = signals.generate_if(FS, (EPOCHS + 3) * VL, [sat], seed=7)
    raw = signals.to_ishort(xf) if fmt == "ci16" else signals.to_ibyte(xf)
    xq = raw.astype(np.float32).view(np.complex64)  # the model is given the quantised samples
    m, ref = model_run("1G", sat, xq)
    assert holds_lock(m, ref)
    (rec, _), _ = device_run(ctx, "1G", sat, raw)
    compare_exact(rec[:, 0], ref, fmt)


def test_four_satellites_through_start_many_with_an_idle_channel(ctx):
    sats = [satellite("1G", k, doppler=d, delay=c, phase=p, cn0=48.0) for k, d, c, p in
            [(2, 1830.0, 207.3, 0.9), (-3, -2410.0, 35.8, 2.2), (0, 640.0, 410.1, 4.0), (1, -3100.0, 120.6, 5.5)]]
    x = signals.generate_if(FS, (EPOCHS + 3) * VL, sats, seed=44)
    refs = []
    for s in sats:
        m, ref = model_run("1G", s, x)
        assert holds_lock(m, ref), s.freq_channel
        refs.append(ref)
    ctx.set_code(CODE_ID, codes.glonass_l1_ca_code_gen_float())
    trk = engine.DllPllVemlTracking(ctx, engine.glonass_l1_ca_trk_conf(FS), 5)
    chans = [0, 1, 3, 4]  # channel 2 stays idle
    trk.start_many([(ch, CODE_ID) + acquisition(s) + (-1, s.prn) for ch, s in zip(chans, sats)])
    rec, done = trk.run(x, 0, EPOCHS)
    assert trk.last_engine() == abi.TRK_ENGINE_PERSIST and done == EPOCHS
    for ch, ref, s in zip(chans, refs, sats):
        compare_exact(rec[:, ch], ref, f"channel {ch} k={s.freq_channel}")
    assert not np.any(np.ascontiguousarray(rec[:, 2]).view(np.uint8)) and trk.channel_state(2)[0] == 0
    trk.close()


def test_nonzero_if(ctx):
    if_hz = -420000
    sat = satellite("1G", 2, f_if_hz=float(if_hz))
    x = signals.generate_if(FS, (EPOCHS + 3) * VL, [sat], seed=9)
    m, ref = model_run("1G", sat, x, if_hz=if_hz)
    assert holds_lock(m, ref)
    (rec, _), _ = device_run(ctx, "1G", sat, x, if_hz=float(if_hz))
    compare_exact(rec[:, 0], ref, "if_hz")


def test_dump_records_and_the_88_byte_file(ctx, tmp_path):
    sat = satellite("1G", -3, doppler=-2410.0)
    x = signals.generate_if(FS, (EPOCHS + 3) * VL, [sat], seed=13)
    m, ref = model_run("1G", sat, x, dump=True)
    assert holds_lock(m, ref) and len(m.dumps) == EPOCHS
    (rec, _, dmp), _ = device_run(ctx, "1G", sat, x, dump=True)
    compare_exact(rec[:, 0], ref, "dump run")
    assert np.all(rec[:, 0]["flags"] == 25)
    want = np.array(m.dumps, abi.TRK_DUMP_DTYPE)
    for f in abi.TRK_DUMP_DTYPE.names:
        assert np.array_equal(dmp[:, 0][f], want[f]), f
    assert not np.any(want["carrier_doppler_rate_hz"]) and not np.any(want["code_freq_rate_chips"])
    assert np.array_equal(want["PRN_start_sample_count"], ref["sample_counter"])  # d_sample_counter: no length added
    (path,) = engine.DllPllVemlTracking.write_dump_files(str(tmp_path / "glo_ch"), rec, dmp, glonass=True)
    got = np.fromfile(path, abi.TRK_DUMP_GLONASS_DTYPE)
    assert got.itemsize == 88 and len(got) == EPOCHS
    for f in abi.TRK_DUMP_GLONASS_DTYPE.names:
        assert np.array_equal(got[f], want[f]), f


def test_loss_of_lock_on_noise(ctx):
    rng = np.random.Generator(np.random.PCG64(7))
    x = (rng.standard_normal(153 * VL) + 1j * rng.standard_normal(153 * VL)).astype(np.complex64)
    sat = signals.Satellite(prn=18, doppler_hz=-900.0, code_delay_chips=0.0, system="GLO_L1")
    start = (1234.5, -900.0, 0, 0)
    m, ref = model_run("1G", sat, x, start=start, max_lock_fail=2)
    assert not m.enable_tracking and len(m.events) == 1 and 33 <= len(ref) < EPOCHS and len(ref) % 11 == 0
    (rec, done), (state, _) = device_run(ctx, "1G", sat, x, start=start, max_carrier_lock_fail=2)
    compare_exact(rec[:, 0], ref, "noise")  # the same number of epochs: lock is lost at the same one
    last = rec[len(ref) - 1, 0]
    assert last["flags"] == (8 | 2) and last["sample_counter"] == m.events[0][1]
    assert np.all(rec[: len(ref) - 1, 0]["flags"] == 9)
    assert state == 0 and done == len(ref) and not np.any(np.ascontiguousarray(rec[len(ref):, 0]).view(np.uint8))  # the channel stopped


def test_glonass_and_gps_trackers_alternate_on_one_context(ctx):
    """The other systems are untouched: a GPS L1 tracker on the generic rotator, run between the GLONASS runs on the
    same context, equals the oracle loop epoch for epoch."""
    sat = satellite("1G", 2)
    x = signals.generate_if(FS, (EPOCHS + 3) * VL, [sat], seed=21)
    m, ref = model_run("1G", sat, x)
    assert holds_lock(m, ref)
    gsat, k, gx, stamp, first, delay, dop = S.sync("GPS", float(FS), 60, rotator_avx=0)
    gref = T.track(k, gx, gsat.code, delay, dop, stamp, first, 60, buffer_first=first)
    ctx.set_code(CODE_ID, codes.glonass_l1_ca_code_gen_float())
    ctx.set_code(CODE_ID + 1, gsat.code)
    glo = engine.DllPllVemlTracking(ctx, engine.glonass_l1_ca_trk_conf(FS), 1)
    gps = engine.DllPllVemlTracking(ctx, dev_conf(k, "GPS"), 1)
    glo.start(0, CODE_ID, *acquisition(sat), prn=sat.prn)
    gps.start(0, CODE_ID + 1, delay, dop, stamp, first)
    parts, gparts = [], []
    for half in range(2):
        parts.append(glo.run(x, 0, EPOCHS // 2)[0][:, 0])
        assert glo.last_engine() == abi.TRK_ENGINE_PERSIST
        gparts.append(gps.run(gx, first, 30)[0][:, 0])
        assert gps.last_engine() == abi.TRK_ENGINE_PERSIST
    compare_exact(np.concatenate(parts), ref, "GLONASS, alternating")
    compare_exact(np.concatenate(gparts), gref, "GPS L1, alternating")
    glo.close()
    gps.close()


def test_avx_rotator_and_unknown_prn_are_refused(ctx):
    for rot in (abi.ROTATOR_AVX,):
        with pytest.raises(abi.GnssHipError) as e:
            engine.DllPllVemlTracking(ctx, engine.glonass_l1_ca_trk_conf(FS, rotator=rot), 1)
        assert e.value.code == abi.E_INVAL and "rotator_dot_prod_32fc_xn" in str(e.value)
    ctx.set_code(CODE_ID, codes.glonass_l1_ca_code_gen_float())
    trk = engine.DllPllVemlTracking(ctx, engine.glonass_l2_ca_trk_conf(FS), 1)
    with pytest.raises(abi.GnssHipError) as e:
        trk.start(0, CODE_ID, 10.0, 0.0, 0, 0, prn=25)
    assert e.value.code == abi.E_INVAL
    trk.close()
