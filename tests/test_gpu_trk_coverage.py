"""Every instantiation of the three persistent closed-loop kernels on the device, against the oracle loop, bit for bit.

test_census_case runs the case table of tests/trk_cases.py (tests/test_trk_cases.py proves on the CPU that it reaches
every instantiation): each case asserts that gnsship_trk_last_plan reports the plan recomputed from the restated
dispatch, that every traced epoch's taps (and data prompt) equal the oracle correlator's on the device's own arguments
(trace_exact), and that every field of every epoch record equals the oracle loop's (compare_exact) — for every
started channel, the idle one staying untouched.  Integer formats carry the type's extreme values in the first three
epochs (trk_cases.planted).

Further: Galileo E1 with track_pilot = 0 (state 2 straight to 4, no secondary code) for 90 epochs on every engine that
has the layout, with the dump records; buffers that end on, and one sample short of, the last epoch's last sample, with
the follow-up run; nine trk_lane rows of which one cannot run, one loses lock and the rest track.

Each case has its own context per scenario, so the LDS replica (sized by the longest code of the context's bank) is
the scenario's and the plan is the one the table computes."""
import numpy as np
import pytest

from gnss_sim_receiver_amd import abi, engine, signals
from oracle import trk as T

import trk_cases as C
from test_gpu_c5_closed_loop import trace_exact
from test_gpu_trk import compare_exact, dev_conf
from test_gpu_trk_b3i import b3i_dev_conf
from test_gpu_trk_l5 import l5_dev_conf

pytestmark = pytest.mark.gpu
KNOBS = ("GNSSHIP_TRK_FAST", "GNSSHIP_TRK_LANE", "GNSSHIP_TRK_THRU", "GNSSHIP_TRK_FAST_LDS", "GNSSHIP_TRK_FAST_PACKED", "GNSSHIP_TRK_ROUNDS")


@pytest.fixture(scope="module")
def contexts(built):
    """One context per scenario, holding that scenario's codes only."""
    made = {}

    def get(scenario):
        if scenario not in made:
            made[scenario] = engine.Context(0)
        return made[scenario]

    yield get
    for c in made.values():
        c.close()


def set_env(monkeypatch, env):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def device_conf(scenario, fs, avx):
    if scenario == "glo":
        return engine.glonass_l1_ca_trk_conf(int(fs))
    k = C.oracle_conf(scenario, fs, avx)
    if scenario == "b3i":
        return b3i_dev_conf(k)
    if scenario == "l5":
        return l5_dev_conf(k)
    return dev_conf(k, "GPS" if scenario == "gps" else "GAL")


def make_tracker(ctx, scenario, fs, avx, n_chans, starts):
    """starts: {channel: (delay, doppler)}."""
    s = C.signal(scenario, fs)
    ctx.set_code(0, s.code)
    if s.data_code is not None:
        ctx.set_code(1, s.data_code)
    trk = engine.DllPllVemlTracking(ctx, device_conf(scenario, fs, avx), n_chans)
    for ch, (delay, dop) in starts.items():
        trk.start(ch, 0, delay, dop, s.stamp, s.first, data_code_id=1 if s.data_code is not None else -1, prn=s.sat.prn)
    return trk


def same_records(a, b, label):
    for f in a.dtype.names:
        same = (a[f] == b[f]) | (np.isnan(a[f]) & np.isnan(b[f])) if a[f].dtype.kind == "f" else a[f] == b[f]
        assert np.all(same), (label, f, int(np.count_nonzero(~same)), a[f][~same][:3], b[f][~same][:3])


@pytest.mark.parametrize("name", C.CASE_IDS)
def test_census_case(contexts, monkeypatch, name):
    c = C.BY_NAME[name]
    set_env(monkeypatch, c.env)
    s = C.signal(c.scenario, c.fs)
    raw = C.planted(c.scenario, c.fs, c.fmt)
    xf = C.as_float(raw)
    chans = C.started_channels(c.n_chans)
    trk = make_tracker(contexts(c.scenario), c.scenario, c.fs, c.avx, c.n_chans, {ch: C.start_args(c.scenario, c.fs, ch) for ch in chans})
    trk.set_trace(True)
    rec, rounds = trk.run(raw, s.first, C.EPOCHS)
    got = trk.last_plan()
    tr = trk.trace(C.EPOCHS)
    trk.close()
    assert got == c.plan(), (name, got, c.plan())
    assert rounds == C.EPOCHS
    for ch in chans:
        label = f"{name} ch{ch}"
        assert trace_exact(tr[:, ch], xf, s.first, s.code, s.data_code, label, avx=c.avx) == C.EPOCHS
        compare_exact(rec[:, ch], C.reference(c.scenario, c.fs, c.fmt, c.avx, ch), label)
    idle = C.IDLE_CHANNEL[c.n_chans]
    assert not np.any(np.ascontiguousarray(rec[:, idle]).view(np.uint8)) and not np.any(tr[:, idle]["n_samples"])


# ---- Galileo E1, the data component alone ------------------------------------------------------------------------
E1D_FS, E1D_EPOCHS = 25e6 / 4, 90
E1D_ENGINES = {
    # name: (avx, knobs, channels, engine, the plan members that tell the variant)
    "trk_fast latency": (True, {"GNSSHIP_TRK_THRU": "0", "GNSSHIP_TRK_LANE": "0"}, 2, abi.TRK_ENGINE_FAST_LATENCY, dict(thru=0, long_plan=1)),
    # five taps have no trk_fast throughput plan (trk_cases.py): the throughput knobs without trk_lane run trk_persist
    "throughput without trk_lane": (True, {"GNSSHIP_TRK_THRU": "1", "GNSSHIP_TRK_LANE": "0"}, 9, abi.TRK_ENGINE_PERSIST, dict(thru=1, avx=1)),
    "trk_lane": (True, {"GNSSHIP_TRK_LANE": "1"}, 9, abi.TRK_ENGINE_LANES, dict(lane_waves=1)),
    "trk_persist avx": (True, {"GNSSHIP_TRK_FAST": "0", "GNSSHIP_TRK_THRU": "0"}, 2, abi.TRK_ENGINE_PERSIST, dict(thru=0, avx=1)),
    "trk_persist generic": (False, {"GNSSHIP_TRK_THRU": "0"}, 2, abi.TRK_ENGINE_PERSIST, dict(thru=0, avx=0)),
}


@pytest.mark.parametrize("which", list(E1D_ENGINES))
def test_e1_data_only_to_state_4(contexts, monkeypatch, which):
    """T.conf("GAL", …, track_pilot=0): five taps, no data prompt, no secondary code — the loop leaves state 2 for 4 at
    the first epoch after the pull-in and stays there.  90 epochs at 6.25 Msps (N = 25000), cf32; taps, records and
    the dump records (test_gpu_trk_b3i.test_dump_records_equal_the_oracle's rule: every field equal).
    Engines: trk_fast's latency form, trk_lane, trk_persist AVX and trk_persist generic.  trk_fast has no throughput
    form for five taps (test_trk_cases.test_five_taps_have_no_throughput_plan), so there is no second trk_fast run:
    "throughput without trk_lane" sets that form's knobs and asserts that the run is trk_persist's AVX form with THRU —
    a second trk_persist AVX run, not a trk_fast one."""
    avx, env, n_chans, want_engine, want_plan = E1D_ENGINES[which]
    set_env(monkeypatch, env)
    sat, k, x, stamp, first, delay, dop = e1d_long()
    k = type(k).from_buffer_copy(k)
    k.rotator_avx = 1 if avx else 0
    ch = n_chans - 1
    ref, rdump = T.track(k, x, sat.code_data, delay, dop, stamp, first, E1D_EPOCHS, buffer_first=first, dump=True, prn=sat.prn)
    assert len(ref) == E1D_EPOCHS and np.count_nonzero(ref["state"] == 4) >= 50 and np.all(ref["state"][-50:] == 4), np.bincount(ref["state"])
    assert set(np.unique(ref["state"]).tolist()) <= {2, 4}
    ctx = contexts("e1d")
    ctx.set_code(0, sat.code_data)
    trk = engine.DllPllVemlTracking(ctx, dev_conf(k, "GAL"), n_chans)
    trk.start(ch, 0, delay, dop, stamp, first, prn=sat.prn)
    trk.set_trace(True)
    rec, rounds, dump = trk.run(x, first, E1D_EPOCHS, dump=True)
    plan = trk.last_plan()
    tr = trk.trace(E1D_EPOCHS)
    state = trk.channel_state(ch)[0]
    trk.close()
    assert plan["engine"] == want_engine and plan["n_taps"] == 5 and plan["data_prompt"] == 0, (which, plan)
    assert {f: plan[f] for f in want_plan} == want_plan, (which, plan)
    assert rounds == E1D_EPOCHS and state == 4
    assert trace_exact(tr[:, ch], x, first, sat.code_data, None, which, avx=avx) == E1D_EPOCHS
    compare_exact(rec[:, ch], ref, which)
    assert np.array_equal(rec[:, ch]["flags"] & 16, ref["flags"] & 16)
    w = (ref["flags"] & 16) != 0
    assert np.count_nonzero(w) > 20
    same_records(dump[w, ch], rdump[w], which)
    for other in range(n_chans - 1):
        assert not np.any(rec[:, other]["flags"])


def e1d_long(_cache={}):
    if not _cache:
        import trk_scenarios as S
        out = S.sync("GAL", E1D_FS, E1D_EPOCHS, track_pilot=0)
        out[2].setflags(write=False)
        _cache["v"] = out
    return _cache["v"]


# ---- buffer edges ------------------------------------------------------------------------------------------------
EDGE_ENGINES = {
    "trk_fast latency": (True, {"GNSSHIP_TRK_THRU": "0", "GNSSHIP_TRK_LANE": "0"}, abi.TRK_ENGINE_FAST_LATENCY),
    "trk_lane": (True, {"GNSSHIP_TRK_LANE": "1"}, abi.TRK_ENGINE_LANES),
    "trk_persist": (False, {"GNSSHIP_TRK_THRU": "0"}, abi.TRK_ENGINE_PERSIST),
}


@pytest.mark.parametrize("short_by", [0, 1])
@pytest.mark.parametrize("which", list(EDGE_ENGINES))
def test_buffer_ends_on_the_last_epochs_last_sample(contexts, monkeypatch, which, short_by):
    """The 3-tap GPS case on CI8 (N = 4300, a 12-sample serial tail that reads the buffer's last samples).  The buffer is
    cut where the oracle's 20th epoch's samples end (short_by = 0: the device runs those 20 epochs) and one sample before
    (19 epochs: the 20th does not fit); records exact, channel_state's next sample the oracle's, and a second run on
    the buffer that continues there resumes exactly — through the end of the 40-epoch reference."""
    avx, env, want_engine = EDGE_ENGINES[which]
    set_env(monkeypatch, env)
    sc, fs, fmt, ch, n_full = "gps", C.RATES["gps"]["short"], "ci8", 1, 20
    s = C.signal(sc, fs)
    raw = C.planted(sc, fs, fmt)
    ref = C.reference(sc, fs, fmt, avx, ch)
    # an epoch correlates vector_length samples from its first one (and then consumes its own code period's length)
    end = int(ref["sample_counter"][n_full - 1]) - s.first + C.vector_length(sc, fs)
    cut = end - short_by
    n_run = n_full - short_by
    # the oracle on the same two buffers
    delay, dop = C.start_args(sc, fs, ch)
    och = T.Channel(C.oracle_conf(sc, fs, avx), s.code, delay, dop, s.stamp, s.first, prn=s.sat.prn)
    xf = C.as_float(raw)
    o1 = och.run(xf[:cut], s.first, C.EPOCHS)
    assert len(o1) == n_run and och.next_sample == int(ref["sample_counter"][n_run])
    trk = make_tracker(contexts(sc), sc, fs, avx, 2, {ch: (delay, dop)})
    r1, done1 = trk.run(raw[:2 * cut], s.first, C.EPOCHS)
    assert trk.last_engine() == want_engine
    state, nxt = trk.channel_state(ch)
    assert done1 == n_run and state == och.state and nxt == och.next_sample
    compare_exact(r1[:, ch], o1, f"{which} cut at {cut}")
    same_records(o1, ref[:n_run], "the oracle on the cut buffer")
    # the continuation: the buffer from the channel's next sample on
    at = nxt - s.first
    r2, done2 = trk.run(raw[2 * at:], nxt, C.EPOCHS)
    o2 = och.run(xf[at:], nxt, C.EPOCHS)
    trk.close()
    assert done2 == len(o2) >= C.EPOCHS - n_run
    compare_exact(r2[:, ch], o2, f"{which} continued at {at}")
    same_records(o2[: C.EPOCHS - n_run], ref[n_run:], "the oracle on the continuation")
    assert not np.any(r1[:, 0]["flags"]) and not np.any(r2[:, 0]["flags"])


# ---- trk_lane: rows of one wave in different conditions -----------------------------------------------------------
def test_lane_mixed_rows_ci16(contexts, monkeypatch):
    """Nine trk_lane rows on CI16 (three workgroups of one wave: four, four and one row): row 2 starts past the
    buffer's end (it cannot run: no record, its state and next sample untouched), row 6 tracks a satellite whose
    signal stops after 25 code periods and loses lock mid-run (the CN0 estimate falls under cn0_min = 38, max_code_lock_fail = 0), the rest track — each
    against its own oracle loop."""
    set_env(monkeypatch, {"GNSSHIP_TRK_LANE": "1"})
    sc, fs, epochs = "gps", C.RATES["gps"]["short"], 60
    n = C.vector_length(sc, fs)
    import trk_scenarios as S
    sat, k, x, stamp, first, delay, dop = S.sync("GPS", fs, epochs, rotator_avx=1, cn0_min=38, max_code_lock_fail=0, cn0_smoother_samples=1,
                                                 cn0_smoother_alpha=0.5)
    other = signals.Satellite(prn=21, doppler_hz=-2210.0, code_delay_chips=611.7, cn0_dbhz=50.0, system="GPS", carrier_phase_rad=2.0,
                              **S.SYNC_PATTERNS["GPS"])
    y = signals.generate_if(fs, len(x), [other], seed=77, start=first).astype(np.complex64)
    noise = signals.generate_if(fs, len(x), [], seed=78, start=first).astype(np.complex64)
    stop = 25 * n
    y[stop:] = noise[stop:]
    raw = signals.to_ishort((x + y).astype(np.complex64))
    xf = raw.astype(np.float32).view(np.complex64)
    delay_o, dop_o = S.acq_delay_for(other, fs, "GPS", 0, first) + 0.2, other.doppler_hz + 15.0
    starts = {}
    for ch in range(9):
        if ch == 6:
            starts[ch] = (other.code, delay_o, dop_o, first)
        elif ch == 2:  # the acquisition stamp and start far past the buffer's last sample
            starts[ch] = (sat.code, delay, dop, first + 10 * len(x))
        else:
            starts[ch] = (sat.code, delay + 0.1 * (ch % 5 - 2), dop + 2.0 * (ch % 7 - 3), first)
    ctx = contexts(sc)
    ctx.set_code(0, sat.code)
    ctx.set_code(2, other.code)
    trk = engine.DllPllVemlTracking(ctx, dev_conf(k, "GPS"), 9)
    for ch, (code, d, f, start) in starts.items():
        trk.start(ch, 2 if ch == 6 else 0, d, f, stamp, start)
    before = trk.channel_state(2)
    rec, rounds = trk.run(raw, first, epochs)
    plan = trk.last_plan()
    states = [trk.channel_state(ch) for ch in range(9)]
    trk.close()
    assert plan["engine"] == abi.TRK_ENGINE_LANES and plan["format"] == abi.FMT_CI16 and plan["lane_waves"] == 1, plan
    assert rounds == epochs
    for ch, (code, d, f, start) in starts.items():
        if ch == 2:
            continue
        och = T.Channel(k, code, d, f, stamp, start)
        ref = och.run(xf, first, epochs)
        compare_exact(rec[:, ch], ref, f"lane row {ch}")
        assert states[ch] == (och.state, och.next_sample), ch
        if ch == 6:
            assert 20 < len(ref) < epochs - 10 and ref["flags"][-1] & 2 and och.state == 0, (len(ref), np.bincount(ref["state"]))
        else:
            assert len(ref) == epochs and och.state in (2, 4)
    assert not np.any(np.ascontiguousarray(rec[:, 2]).view(np.uint8)) and states[2] == before and before[0] == 2
