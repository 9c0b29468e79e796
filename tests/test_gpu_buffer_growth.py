"""The device buffers a handle grows on demand (gnsship::DevBuf, csrc/host_api.h), on the GPU: one handle goes through
a small call, a larger one that forces every run-sized buffer to grow, and the small one again; every result must be
bit-equal to the same call on a fresh handle, which never held another size.  Success paths only: what a failed grow
leaves behind is tests/test_dev_buf.py's subject.

Handles that carry state from run to run (tracking channels, filter histories, the LNAV frame synchroniser) are put
back to their first state before each call, so the fresh handle is the whole reference."""
import numpy as np
import pytest

from gnss_sim_receiver_amd import abi, codes, engine, signals

pytestmark = pytest.mark.gpu

FS, VL = 4e6, 4000


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------- tracking
@pytest.fixture(scope="module")
def trk_case(ctx):
    sats = signals.random_sky(2, seed=1)
    x = signals.generate_if(FS, 6 * VL, sats, seed=3)
    starts = []
    for ch, s in enumerate(sats):
        ctx.set_code(840 + ch, s.code)
        starts.append((ch, 840 + ch, (s.code_delay_chips / s.code_freq()) * FS + 0.2, s.doppler_hz + 10.0, 0, 0, -1, s.prn))
    return x, starts


def trk_step(trk, x, starts, rounds, trace):
    """One start_many and one host-staged run of `rounds` epochs over a buffer that just holds them (the pull-in skips up
    to two code periods)."""
    trk.set_trace(trace)
    for ch in range(trk.max_channels):
        trk.stop(ch)
    trk.start_many(starts)
    rec, done, dump = trk.run(x[: (rounds + 2) * VL + 200], 0, rounds, dump=True)
    return rec, done, dump, (trk.trace(rounds) if trace else None)


# persistent loop (generic rotator: trk_persist.hip) and, with GNSSHIP_TRK_ROUNDS=1, the round-based loop
@pytest.mark.parametrize("rounds_loop", [False, True], ids=["persistent", "round-based"])
def test_tracking_records_dump_trace_and_start_staging(ctx, trk_case, monkeypatch, rounds_loop):
    x, starts = trk_case
    if rounds_loop:
        monkeypatch.setenv("GNSSHIP_TRK_ROUNDS", "1")
    conf = abi.TrkConf.defaults(abi.SYS_GPS_L1CA, FS, VL, rotator=abi.ROTATOR_GENERIC)
    want_engine = abi.TRK_ENGINE_ROUNDS if rounds_loop else abi.TRK_ENGINE_PERSIST
    # (channels started, max_rounds, trace): 1 → 3 → 1 rounds, 1 → 2 → 1 channels, then the trace buffer (persistent loop only)
    steps = [(starts[:1], 1, False), (starts, 3, False), (starts[:1], 1, False)]
    if not rounds_loop:
        steps += [(starts[:1], 1, True), (starts, 3, True), (starts[:1], 1, True)]
    reused = engine.DllPllVemlTracking(ctx, conf, 2)
    try:
        for i, (st, rounds, trace) in enumerate(steps):
            fresh = engine.DllPllVemlTracking(ctx, conf, 2)
            try:
                want = trk_step(fresh, x, st, rounds, trace)
                assert fresh.last_engine() == want_engine
            finally:
                fresh.close()
            got = trk_step(reused, x, st, rounds, trace)
            assert reused.last_engine() == want_engine
            label = f"step {i}: {len(st)} channels, {rounds} rounds, trace {trace}"
            assert want[1] == rounds and got[1] == rounds, label
            assert np.all(want[0][:, : len(st)]["flags"] & 8), label  # every started channel ran every epoch
            assert same(got[0], want[0]), label
            written = (want[0]["flags"] & abi.TRK_FLAG_DUMP) != 0  # log_data wrote these; the others are not defined
            assert same(got[2][written], want[2][written]), label
            if trace:
                assert same(got[3], want[3]), label
    finally:
        reused.close()


# ---------------------------------------------------------------------------------------------------- batched correlator
@pytest.mark.parametrize("flags", [abi.JOB_ROTATOR_AVX, 0, abi.JOB_HIGH_DYN], ids=["standard", "serial-order", "high-dynamics"])
def test_batch_set_jobs_small_large_small(ctx, flags):
    sat = signals.random_sky(1, seed=5)[0]
    x = signals.generate_if(FS, 9 * VL, [sat], seed=6)
    ctx.set_code(850, sat.code)
    jobs = signals.truth_jobs(sat, FS, 5, VL, [-0.5, 0.0, 0.5], 850)
    jobs["flags"] = flags
    jobs[3]["n_samples"] = 2 * VL + 193  # three chunks, the last one short
    assert int(jobs[3]["sample_offset"]) + int(jobs[3]["n_samples"]) <= len(x)
    buf = ctx.upload(x)

    def run(b, js):
        b.set_jobs(js, len(x))
        b.launch(buf, abi.FMT_CF32)
        return b.results()

    reused = engine.CorrelatorBatch(ctx, 5)
    try:
        for js in (jobs[:1], jobs, jobs[:1]):
            fresh = engine.CorrelatorBatch(ctx, 5)
            try:
                want = run(fresh, js)
            finally:
                fresh.close()
            assert np.all(np.abs(want[:, 1]) > 0), len(js)  # the prompt tap of every job correlated something
            assert same(run(reused, js), want), len(js)
    finally:
        reused.close()
        buf.free()


# ---------------------------------------------------------------------------------------------------- acquisition
def test_acquisition_grid_one_two_one_prns_and_a_wider_grid(ctx):
    fs, n = 4000000, 4000
    sats = [signals.Satellite(prn=9, doppler_hz=1234.0, code_delay_chips=321.4, cn0_dbhz=46.0),
            signals.Satellite(prn=17, doppler_hz=-2100.0, code_delay_chips=100.3, cn0_dbhz=46.0)]
    sig = signals.generate_if(fs, n, sats, seed=4)

    def make():
        acq = engine.PcpsAcquisition(ctx, fs, n, 5000, 500, 0, True, max_prns=2)
        for slot, s in enumerate(sats):
            acq.set_local_code(codes.gps_l1_ca_code_gen_complex_sampled(s.prn, fs), slot)
        return acq

    def run(acq, n_prns, step):
        if step != acq.conf.doppler_step:
            acq.set_grid(5000, step, 0)  # another number of bins: the grid is released and grown again
            acq.conf.doppler_step = step
        res, grid = acq.run(sig, n_prns=n_prns, want_grid=True)
        return np.array([(r.doppler_index, r.code_index, r.peak, r.input_power, r.test_statistic) for r in res], np.float64), grid

    reused = make()
    try:
        for n_prns, step in ((1, 500), (2, 500), (1, 500), (2, 250), (1, 500)):
            fresh = make()
            try:
                want = run(fresh, n_prns, step)
            finally:
                fresh.close()
            got = run(reused, n_prns, step)
            assert want[1].shape == (n_prns, 10000 // step, n) and np.all(want[1].max(axis=(1, 2)) > 0), (n_prns, step)
            assert same(got[0], want[0]) and same(got[1], want[1]), (n_prns, step)
    finally:
        reused.close()


# ---------------------------------------------------------------------------------------------------- input stage
def host_input_lengths(n_in):
    rng = np.random.default_rng(0x6E550021)
    x = (rng.standard_normal(4 * n_in) + 1j * rng.standard_normal(4 * n_in)).astype(np.complex64)
    taps = rng.standard_normal(7).astype(np.float32)
    return x, taps, (n_in, 4 * n_in, n_in)


def test_conditioner_host_input_small_large_small(ctx):
    x, taps, lengths = host_input_lengths(1000)
    band = (250_000, 2, taps)
    reused = engine.SignalConditioner(ctx, FS, [band], len(x))
    try:
        for n in lengths:
            fresh = engine.SignalConditioner(ctx, FS, [band], len(x))
            try:
                (want,) = fresh.run(x[:n])
            finally:
                fresh.close()
            reused.reset(0)
            (got,) = reused.run(x[:n])
            assert len(want) == n // 2 and np.all(want != 0), n
            assert same(got, want), n
    finally:
        reused.close()


def test_acq_resampler_host_input_small_large_small(ctx):
    x, taps, lengths = host_input_lengths(1000)
    reused = engine.AcqResampler(ctx, taps, 2, len(x))
    try:
        for n in lengths:
            fresh = engine.AcqResampler(ctx, taps, 2, len(x))
            try:
                want = fresh.run(x[:n])
            finally:
                fresh.close()
            reused.reset()
            got = reused.run(x[:n])
            assert len(want) == n // 2 and np.all(want != 0), n
            assert same(got, want), n
    finally:
        reused.close()


# ---------------------------------------------------------------------------------------------------- telemetry (LNAV)
def test_lnav_host_symbols_one_max_one_rounds(ctx):
    channels, max_rounds = 2, 64
    rng = np.random.default_rng(0x6E550022)
    sym = np.where(rng.random((max_rounds, channels)) < 0.5, -1.0, 1.0).astype(np.float32)
    valid = (rng.random((max_rounds, channels)) < 0.9).astype(np.uint8)     # all three staging buffers: symbols,
    flags180 = (rng.random((max_rounds, channels)) < 0.5).astype(np.uint8)  # validity mask, second mask
    reused = engine.gps_l1_ca_telemetry(ctx, channels, max_rounds)
    try:
        for n in (1, max_rounds, 1):
            fresh = engine.gps_l1_ca_telemetry(ctx, channels, max_rounds)
            try:
                want = fresh.run_symbols(sym[:n], valid[:n], flags180[:n])
                state = [fresh.state(ch) for ch in range(channels)]
            finally:
                fresh.close()
            for ch in range(channels):
                reused.new_channel(ch)
            got = reused.run_symbols(sym[:n], valid[:n], flags180[:n])
            assert want.tow_ms.shape == (n, channels), n
            for name, g, w in zip(want._fields, got, want):
                assert same(g, w), (n, name)
            assert [reused.state(ch) for ch in range(channels)] == state, n
    finally:
        reused.close()
