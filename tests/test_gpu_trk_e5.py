"""Galileo E5a / E5b tracking (GNSSHIP_SYS_GAL_E5A / _E5B) on the device vs the oracle loop configured with the
signals' constants (tests/e5_scenarios.py; the scenarios' own conditions are asserted in
tests/test_oracle_trk_e5.py).

  pilot mode      3 taps on the Q primary + the I primary on the data prompt (the GPS L5 layout); the 100-chip
                  synchronisation pattern is the channel's own, selected by start's prn; the valid symbols'
                  prompt_i / prompt_q are exchanged (d_interchange_iq) — the oracle has no such path, so
                  e5_scenarios.exchanged() swaps them in its records; dump records are not exchanged
  data-only mode  3 taps on the I primary (the BeiDou B3I layout), the I secondary code synchronised and removed

Every comparison is test_gpu_trk.compare_exact's rule — every epoch-record field equal, NaN equal to NaN — and
every test asserts the engine that ran (gnsship_trk_last_engine).  The device configuration carries the library's
default slope / spc / y_intercept: the engine derives the values the block sets (1, early_late_space_chips, 1).
"""
import functools

import numpy as np
import pytest

from gnss_sim_receiver_amd import abi, engine, signals
from oracle import trk as T

import e5_scenarios as E
import l5_scenarios as L5
from test_gpu_trk import SHARED, compare_exact
from test_gpu_trk_l5 import l5_dev_conf

pytestmark = pytest.mark.gpu
FS_A, FS_B = 12.5e6, 8.184e6  # N = 12500 (trk_fast's long-epoch form) and N = 8184 (under one sample per chip)
DERIVED = ("slope", "spc", "y_intercept")
SYSTEM = {"a": abi.SYS_GAL_E5A, "b": abi.SYS_GAL_E5B}
BANDS = ["a", "b"]


def e5_dev_conf(band, k, extend=None):
    make = engine.galileo_e5a_trk_conf if band == "a" else engine.galileo_e5b_trk_conf
    c = make(k.fs_in, track_pilot=k.track_pilot)
    assert c.vector_length == k.vector_length and c.system == SYSTEM[band]
    for f in SHARED:
        if f not in DERIVED:
            setattr(c, f, getattr(k, f))
    if extend is not None:  # as configured, before the adapter's limits: the engine applies them
        c.extend_correlation_symbols = extend
    c.rotator = abi.ROTATOR_AVX if k.rotator_avx else abi.ROTATOR_GENERIC
    return c


@functools.lru_cache(maxsize=None)
def signal(band, fs, prn):
    """(sat, x, stamp, first, delay, dop): the scenario's samples, which do not depend on the loop configuration."""
    sat, _, x, stamp, first, delay, dop = E.sync(band, fs, prn=prn)
    x.setflags(write=False)
    return sat, x, stamp, first, delay, dop


@functools.lru_cache(maxsize=None)
def scenario(band, fs=FS_A, pilot=True, prn=11, avx=1, ext=1, fll=0):
    """(sat, k, x, stamp, first, delay, dop, oracle records, pilot, band): computed once, shared, never modified."""
    sat, x, stamp, first, delay, dop = signal(band, fs, prn)
    k = E.conf(band, fs, prn, pilot, rotator_avx=avx, extend_correlation_symbols=ext, enable_fll_pull_in=fll)
    ref = E.track(sat, k, x, stamp, first, delay, dop, E.EPOCHS[band], pilot=pilot)
    ref.setflags(write=False)
    assert len(ref) == E.EPOCHS[band] and np.any(ref["state"][:230] == 4) and not np.any(ref["flags"] & 2)
    return sat, k, x, stamp, first, delay, dop, ref, pilot, band


def start_one(ctx, trk, sc, ch, base=80):
    sat, k, x, stamp, first, delay, dop, ref, pilot, band = sc
    code, data = E.replicas(sat, pilot)
    ctx.set_code(base, code)
    if data is not None:
        ctx.set_code(base + 1, data)
    trk.start(ch, base, delay, dop, stamp, first, data_code_id=base + 1 if data is not None else -1, prn=sat.prn)


def run_one(ctx, sc, sig=None, n_ch=2, ch=1, dump=False, extend=None):
    sat, k, x, stamp, first, delay, dop, ref, pilot, band = sc
    trk = engine.DllPllVemlTracking(ctx, e5_dev_conf(band, k, extend), n_ch)
    start_one(ctx, trk, sc, ch)
    out = trk.run(x if sig is None else sig, first, len(ref), dump=dump)
    eng = trk.last_engine()
    trk.close()
    return out, eng


# ---- pilot mode on every engine -------------------------------------------------------------------------------

@pytest.mark.parametrize("band", BANDS)
def test_pilot_fast_long_epoch_form(ctx, band):
    """12.5 Msps, N = 12500: trk_fast on the two sign-bit replicas, channel 0 left idle."""
    sc = scenario(band)
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    assert rounds == len(sc[7])
    compare_exact(rec[:, 1], sc[7], f"E5{band} pilot trk_fast")
    assert not np.any(rec[:, 0]["flags"])


@pytest.mark.parametrize("band,prn", [("a", 36), ("b", 50)])
def test_pilot_fast_latency_wave_count(ctx, band, prn):
    """8.184 Msps, N = 8184 < 10000 (under one sample per chip): trk_fast with the latency form's wave count, on other
    PRN rows than the 12.5 Msps cases (E5a 36; E5b 50, the table's last row)."""
    sc = scenario(band, FS_B, prn=prn)
    assert sc[1].vector_length == 8184
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], sc[7], f"E5{band} pilot 8.184 Msps")


@pytest.mark.parametrize("band", BANDS)
def test_pilot_fast_throughput_form(ctx, monkeypatch, band):
    """GNSSHIP_TRK_THRU=1 without trk_lane: trk_fast's throughput form, which reads the pattern from the
    parameter block's PRN row instead of an LDS copy."""
    monkeypatch.setenv("GNSSHIP_TRK_THRU", "1")
    monkeypatch.setenv("GNSSHIP_TRK_LANE", "0")
    sc = scenario(band)
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_FAST_THROUGHPUT, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], sc[7], f"E5{band} pilot trk_fast throughput")


@pytest.mark.parametrize("band", BANDS)
def test_pilot_lanes(ctx, monkeypatch, band):
    monkeypatch.setenv("GNSSHIP_TRK_LANE", "1")
    sc = scenario(band)
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_LANES, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], sc[7], f"E5{band} pilot trk_lane")
    assert not np.any(rec[:, 0]["flags"])


@pytest.mark.parametrize("band", BANDS)
def test_pilot_persist_avx(ctx, monkeypatch, band):
    """GNSSHIP_TRK_FAST=0: trk_persist.hip with the AVX rotator (chains_avx for this tap layout)."""
    monkeypatch.setenv("GNSSHIP_TRK_FAST", "0")
    sc = scenario(band)
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_PERSIST, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], sc[7], f"E5{band} pilot trk_persist avx")


@pytest.mark.parametrize("band", BANDS)
def test_pilot_persist_generic_rotator(ctx, band):
    sc = scenario(band, avx=0)
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_PERSIST, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], sc[7], f"E5{band} pilot trk_persist generic")


# ---- data-only mode -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("packed", [1, 0])
def test_data_only_fast(ctx, monkeypatch, band, packed):
    """track_pilot = 0: trk_fast on the I primary held as sign bits, and (GNSSHIP_TRK_FAST_PACKED=0) as floats."""
    if not packed:
        monkeypatch.setenv("GNSSHIP_TRK_FAST_PACKED", "0")
    sc = scenario(band, pilot=False)
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], sc[7], f"E5{band} data-only trk_fast packed={packed}")
    assert not np.any(rec[:, 0]["flags"])


@pytest.mark.parametrize("band", BANDS)
def test_data_only_lanes(ctx, monkeypatch, band):
    monkeypatch.setenv("GNSSHIP_TRK_LANE", "1")
    sc = scenario(band, pilot=False)
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_LANES, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], sc[7], f"E5{band} data-only trk_lane")


# ---- input formats, loop variants, dumps ----------------------------------------------------------------------

@pytest.mark.parametrize("band", BANDS)
def test_ci8_input(ctx, band):
    """CI8 input in pilot mode (CF32 is every other test): the oracle gets the same quantised samples as floats."""
    sat, k, x, stamp, first, delay, dop, _, pilot, _ = scenario(band)
    raw = signals.to_ibyte(x)
    xq = raw.astype(np.float32).view(np.complex64)
    ref = E.track(sat, k, x, stamp, first, delay, dop, E.EPOCHS[band], samples=xq)
    assert np.any(ref["state"][:230] == 4) and not np.any(ref["flags"] & 2) and np.count_nonzero(ref["flags"] & 1) >= 20
    (rec, rounds), eng = run_one(ctx, (sat, k, x, stamp, first, delay, dop, ref, pilot, band), sig=raw)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], ref, f"E5{band} ci8")


@pytest.mark.parametrize("band", BANDS)
def test_pilot_extended_integration(ctx, band):
    """extend_correlation_symbols = 4 in pilot mode: state-3 coherent epochs between narrow updates."""
    sc = scenario(band, ext=4)
    st = sc[7]["state"]
    assert sc[1].extend_correlation_symbols == 4 and np.sum(st == 3) >= 3 * 10 and np.sum(st == 4) >= 10
    (rec, rounds), eng = run_one(ctx, sc, n_ch=1, ch=0)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 0], sc[7], f"E5{band} pilot x4")


def test_data_only_extension_is_clamped_to_the_i_secondary_length(ctx):
    """extend_correlation_symbols = 25 in E5a data-only mode runs as 20 (galileo_e5a_dll_pll_tracking.cc:47-58)."""
    sc = scenario("a", pilot=False, ext=25)
    st = sc[7]["state"]
    assert sc[1].extend_correlation_symbols == 20 and np.sum(st == 3) >= 19 * 10
    (rec, rounds), eng = run_one(ctx, sc, n_ch=1, ch=0, extend=25)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 0], sc[7], "E5a data-only x25 -> x20")


def test_fll_pull_in(ctx):
    """enable_fll_pull_in: the FLL-assisted carrier loop over the scenario's ten pull-in epochs."""
    sc = scenario("a", fll=1)
    plain = scenario("a")
    assert not np.array_equal(sc[7]["carrier_doppler_hz"][:12], plain[7]["carrier_doppler_hz"][:12])
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], sc[7], "E5a pilot fll pull-in")


@pytest.mark.parametrize("band", BANDS)
def test_dump_records_equal_the_oracle_and_are_not_exchanged(ctx, band):
    """log_data's records in pilot mode: written on the same epochs, every field equal to the oracle's own — the
    prompt as log_data wrote it, not exchanged — while the epoch records' symbols are."""
    sat, k, x, stamp, first, delay, dop, _, pilot, _ = scenario(band)
    ref, rdump = E.track(sat, k, x, stamp, first, delay, dop, E.EPOCHS[band], dump=True)
    (rec, rounds, dump), eng = run_one(ctx, (sat, k, x, stamp, first, delay, dop, ref, pilot, band), n_ch=1, ch=0, dump=True)
    assert eng == abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 0], ref, f"E5{band} dump run")
    ran = (rec[:, 0]["flags"] & 8) != 0
    d_rec, d_dump = rec[ran, 0], dump[ran, 0]
    assert np.array_equal(d_rec["flags"] & 16, ref["flags"] & 16)
    w = (ref["flags"] & 16) != 0
    a, b = d_dump[w], rdump[w]
    assert len(a) > 20
    for f in abi.TRK_DUMP_DTYPE.names:
        same = (a[f] == b[f]) | (np.isnan(a[f]) & np.isnan(b[f])) if a[f].dtype.kind == "f" else a[f] == b[f]
        assert np.all(same), (f, int(np.count_nonzero(~same)), a[f][~same][:3], b[f][~same][:3])
    assert np.all(a["PRN"] == sat.prn)


# ---- the pattern belongs to the channel -----------------------------------------------------------------------

PRNS4 = ((3, -2310.0, 9911.7, 0.3), (11, 640.5, 17.2, 2.1), (29, 3875.0, 5120.4, 4.0), (50, -95.0, 7000.9, 5.5))


@functools.lru_cache(maxsize=None)
def four_satellites(band="b", fs=FS_A):
    """Four satellites of four PRNs in one buffer, with what each channel is started with and its own oracle run."""
    epochs = E.EPOCHS[band]
    sats = [E.satellite(band, prn=p, dop=d, delay_chips=c, cn0=48.0, phase=ph) for p, d, c, ph in PRNS4]
    first = E.first_sample(fs)
    ks = [E.conf(band, fs, s.prn, True, rotator_avx=1) for s in sats]
    x = signals.generate_if(fs, ks[0].vector_length * (epochs + 5), sats, seed=21, start=first)
    x.setflags(write=False)
    starts = [(E.acq_delay_for(s, fs, 0, first) + 0.3 - 0.2 * ch, s.doppler_hz - 20.0 + 10.0 * ch) for ch, s in enumerate(sats)]
    refs = [E.track(s, ks[ch], x, 0, first, starts[ch][0], starts[ch][1], epochs) for ch, s in enumerate(sats)]
    for r in refs:
        assert len(r) == epochs and np.any(r["state"][:230] == 4) and not np.any(r["flags"] & 2) and np.count_nonzero(r["flags"] & 1) >= 20
    return sats, ks, x, first, starts, refs


def load_codes(ctx, sats, base=90):
    for ch, s in enumerate(sats):
        ctx.set_code(base + 2 * ch, s.code)
        ctx.set_code(base + 2 * ch + 1, s.code_data)


@pytest.mark.parametrize("engine_env,want", [({}, abi.TRK_ENGINE_FAST_LATENCY), ({"GNSSHIP_TRK_LANE": "1"}, abi.TRK_ENGINE_LANES),
                                             ({"GNSSHIP_TRK_FAST": "0"}, abi.TRK_ENGINE_PERSIST)])
def test_four_channels_of_four_prns_from_one_start_many(ctx, monkeypatch, engine_env, want):
    """Each channel synchronises on its own satellite's secondary code: with one pattern per system at most one of
    the four would leave state 2."""
    for name, v in engine_env.items():
        monkeypatch.setenv(name, v)
    sats, ks, x, first, starts, refs = four_satellites()
    assert len({E.BAND["b"][3](s.prn) for s in sats}) == 4
    trk = engine.DllPllVemlTracking(ctx, e5_dev_conf("b", ks[0]), len(sats))
    load_codes(ctx, sats)
    trk.start_many([(ch, 90 + 2 * ch, starts[ch][0], starts[ch][1], 0, first, 91 + 2 * ch, s.prn) for ch, s in enumerate(sats)])
    rec, rounds = trk.run(x, first, len(refs[0]))
    eng = trk.last_engine()
    trk.close()
    assert eng == want, abi.TRK_ENGINE_NAMES[eng]
    for ch, s in enumerate(sats):
        compare_exact(rec[:, ch], refs[ch], f"E5b ch{ch} PRN {s.prn}")


def test_channel_restarted_on_another_prn_in_the_same_handle(ctx):
    """Channel 0 tracks PRN 3 for 130 epochs, is stopped and restarted on PRN 29 from the scenario's start: the
    second run equals PRN 29's oracle run (its own pattern, not the one the channel held before)."""
    sats, ks, x, first, starts, refs = four_satellites()
    trk = engine.DllPllVemlTracking(ctx, e5_dev_conf("b", ks[0]), 2)
    load_codes(ctx, sats)
    trk.start(0, 90, starts[0][0], starts[0][1], 0, first, data_code_id=91, prn=sats[0].prn)
    rec_a, _ = trk.run(x, first, 130)
    compare_exact(rec_a[:, 0], refs[0][:130], "E5b PRN 3 before the restart")
    assert trk.channel_state(0)[0] == 4
    trk.stop(0)
    trk.start(0, 94, starts[2][0], starts[2][1], 0, first, data_code_id=95, prn=sats[2].prn)
    rec_b, _ = trk.run(x, first, len(refs[2]))
    assert trk.last_engine() == abi.TRK_ENGINE_FAST_LATENCY
    trk.close()
    compare_exact(rec_b[:, 0], refs[2], "E5b PRN 29 after the restart")


def test_e5a_and_l5_trackers_on_one_context(ctx):
    """An E5a tracker and a GPS L5 tracker (same tap layout, same kernels, the system's own NH20 pattern) run
    alternately on one context: the L5 records still equal their oracle, and so do the E5a ones."""
    e5 = scenario("a")
    sat5, k5, x5, stamp5, first5, delay5, dop5 = L5.sync(FS_A, 120, rotator_avx=1)
    ref5 = T.track(k5, x5, sat5.code, delay5, dop5, stamp5, first5, 120, data_code=sat5.code_data, buffer_first=first5)
    assert ref5["state"][-1] == 4
    ta = engine.DllPllVemlTracking(ctx, e5_dev_conf("a", e5[1]), 1)
    t5 = engine.DllPllVemlTracking(ctx, l5_dev_conf(k5), 1)
    start_one(ctx, ta, e5, 0, base=80)
    ctx.set_code(84, sat5.code)
    ctx.set_code(85, sat5.code_data)
    t5.start(0, 84, delay5, dop5, stamp5, first5, data_code_id=85, prn=sat5.prn)
    n = len(e5[7])
    cut = 200
    rec_a1, _ = ta.run(e5[2], e5[4], cut)
    rec_5a, _ = t5.run(x5, first5, 60)
    rec_a2, _ = ta.run(e5[2], e5[4], n - cut)
    rec_5b, _ = t5.run(x5, first5, 60)
    assert ta.last_engine() == abi.TRK_ENGINE_FAST_LATENCY and t5.last_engine() == abi.TRK_ENGINE_FAST_LATENCY
    ta.close()
    t5.close()
    compare_exact(np.concatenate([rec_5a[:, 0], rec_5b[:, 0]]), ref5, "L5 beside E5a")
    compare_exact(np.concatenate([rec_a1[:, 0], rec_a2[:, 0]]), e5[7], "E5a beside L5")


# ---- rejection ------------------------------------------------------------------------------------------------

def test_prn_without_a_pattern_is_rejected_and_leaves_the_other_channels_running(ctx):
    """start with PRN 51 (and 0, and through start_many) returns E_INVAL before any device state changes: channel
    0, half way through its run, finishes it equal to the oracle, and the refused channel stays idle."""
    sc = scenario("b")
    sat, k, x, stamp, first, delay, dop, ref, pilot, band = sc
    trk = engine.DllPllVemlTracking(ctx, e5_dev_conf("b", k), 2)
    start_one(ctx, trk, sc, 0)
    rec_a, _ = trk.run(x, first, 120)
    for prn in (51, 0, -3):
        with pytest.raises(abi.GnssHipError) as e:
            trk.start(1, 80, delay, dop, stamp, first, data_code_id=81, prn=prn)
        assert e.value.code == abi.E_INVAL and "PRN" in str(e.value)
    with pytest.raises(abi.GnssHipError) as e:  # one bad entry refuses the whole transaction, channel 0's restart included
        trk.start_many([(0, 80, delay + 7.0, dop, stamp, first, 81, sat.prn), (1, 80, delay, dop, stamp, first, 81, 51)])
    assert e.value.code == abi.E_INVAL
    assert trk.channel_state(1)[0] == 0
    rec_b, _ = trk.run(x, first, len(ref) - 120)
    trk.close()
    assert not np.any(rec_a[:, 1]["flags"]) and not np.any(rec_b[:, 1]["flags"])
    compare_exact(np.concatenate([rec_a[:, 0], rec_b[:, 0]]), ref, "E5b beside a refused start")


def test_e5a_pilot_prn_48_is_rejected_data_only_accepts_it(ctx):
    """The E5a-Q secondary table ends at PRN 47 (as the reference's): pilot tracking refuses 48..50; data-only
    tracking, which needs no pilot pattern, takes every PRN of the 50."""
    sc = scenario("a")
    sat, k, x, stamp, first, delay, dop, ref, pilot, band = sc
    trk = engine.DllPllVemlTracking(ctx, e5_dev_conf("a", k), 1)
    ctx.set_code(80, sat.code)
    ctx.set_code(81, sat.code_data)
    for prn in (48, 50, 51):
        with pytest.raises(abi.GnssHipError) as e:
            trk.start(0, 80, delay, dop, stamp, first, data_code_id=81, prn=prn)
        assert e.value.code == abi.E_INVAL
    trk.start(0, 80, delay, dop, stamp, first, data_code_id=81, prn=47)
    trk.close()
    kd = E.conf("a", FS_A, 11, False, rotator_avx=1)
    trk = engine.DllPllVemlTracking(ctx, e5_dev_conf("a", kd), 1)
    trk.start(0, 81, delay, dop, stamp, first, prn=50)
    with pytest.raises(abi.GnssHipError):
        trk.start(0, 81, delay, dop, stamp, first, prn=51)
    trk.close()


# ---- the round-based loop -------------------------------------------------------------------------------------

@pytest.mark.parametrize("band,pilot", [("a", True), ("b", True), ("a", False)])
def test_round_loop(ctx, monkeypatch, band, pilot):
    """GNSSHIP_TRK_ROUNDS=1 with the generic rotator: the round-based loop (trk_kernel.hip), one step launch and one
    correlator launch per epoch.  For these two systems the round loop correlates with the serial-order correlator
    (corr_serial.hip: the generic rotator's phasor chain and serial float sums), not with the batch correlator's
    chunked sums the older systems keep, so its records equal the oracle's in every field as the persistent
    engines' do.  Channel 0 is idle: its job slot is skipped every round."""
    monkeypatch.setenv("GNSSHIP_TRK_ROUNDS", "1")
    sc = scenario(band, pilot=pilot, avx=0)
    (rec, rounds), eng = run_one(ctx, sc)
    assert eng == abi.TRK_ENGINE_ROUNDS, abi.TRK_ENGINE_NAMES[eng]
    compare_exact(rec[:, 1], sc[7], f"E5{band} pilot={pilot} round loop")
    assert not np.any(rec[:, 0]["flags"])


def test_round_loop_four_channels_of_four_prns(ctx, monkeypatch):
    """The per-channel pattern on the round loop: four PRNs from one start_many, generic rotator."""
    monkeypatch.setenv("GNSSHIP_TRK_ROUNDS", "1")
    sats, ks, x, first, starts, _ = four_satellites()
    kg = [E.conf("b", FS_A, s.prn, True, rotator_avx=0) for s in sats]
    trk = engine.DllPllVemlTracking(ctx, e5_dev_conf("b", kg[0]), len(sats))
    load_codes(ctx, sats)
    trk.start_many([(ch, 90 + 2 * ch, starts[ch][0], starts[ch][1], 0, first, 91 + 2 * ch, s.prn) for ch, s in enumerate(sats)])
    rec, rounds = trk.run(x, first, E.EPOCHS["b"])
    eng = trk.last_engine()
    trk.close()
    assert eng == abi.TRK_ENGINE_ROUNDS, abi.TRK_ENGINE_NAMES[eng]
    for ch, s in enumerate(sats):
        ref = E.track(s, kg[ch], x, 0, first, starts[ch][0], starts[ch][1], E.EPOCHS["b"])
        assert np.any(ref["state"][:230] == 4) and not np.any(ref["flags"] & 2)
        compare_exact(rec[:, ch], ref, f"E5b round loop ch{ch} PRN {s.prn}")
